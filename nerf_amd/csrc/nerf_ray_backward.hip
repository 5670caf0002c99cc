// Backward of the fused renderer w.r.t. the RAYS (gfx950 only): dL/d rays_o, dL/d rays_d for pose refinement — what
// PyTorch autograd gives the reference through NeRF.render_rays / NeRF.forward (nerf/model.py:544-594, :596-668).
// nerf_hip_render_backward_rays runs the launches of nerf_hip_render_backward (the weight gradient only when the
// parameters are trained), then two of its own, no float atomics, bitwise reproducible:
//   1. nerf_ray_grad_kernel — one wave per (padded ray, 16-sample chunk), like the data gradient:
//      dL/dh = dY_0 W_0 as an exact-fp32 MFMA product ([16 samples x hidden] . [hidden x 96], W_0 staged in LDS);
//      the encoding's backward from the saved h (it holds exp(-v/2) sin y AND exp(-v/2) cos y: no transcendental),
//      the frustum's (mean = o + t_mean d, cov_c = t_var d_c^2 + r_var (1 - d_c^2 / max(|d|^2, 1e-10))), the
//      distance route of the compositing (dist_i = |mean_{i+1} - mean_i|, render_rays only) and the `mean` output
//      of NeRF.forward; a DPP row sum over the chunk's samples -> one partial of 6 floats per (ray, chunk).
//   2. nerf_ray_sum_kernel — per ray, the chunk partials summed in chunk order.
// DESIGN.md ("Ray gradients") has the derivation.
#include "nerf_backward_common.h"

using namespace nerf_layout;
using namespace nerf_device;

namespace {

constexpr int kRayWaves = 8;                // waves per workgroup (W_0 in LDS is shared by them)
constexpr int kW0Stride = 100;              // floats between two rows of W_0 in LDS: 4 rows apart = 16 banks apart
constexpr int kRayPartialFloats = 8;        // per (ray slot, chunk): d rays_o[3], d rays_d[3], 2 unused
constexpr int kFeatTiles = kEncIn / 16;     // 16-feature tiles of dL/dh

struct RayArgs {
    NerfHipRenderArgs a;
    const float* w0;            // [hidden][enc_in]
    const float* d_mean;        // [n_rays][P][3] or null
    float* partial;             // [items][kRayPartialFloats]
    float* d_rays_o;            // [n_rays][3] or null
    float* d_rays_d;            // [n_rays][3] or null
    TrainLayout L;
    int32_t P, chunks;
    int32_t width;              // floats per saved dY row (256, or 128 for a network that trains at 8 tiles)
    int32_t ctiles;             // register tiles of dY_0 the data gradient wrote (nerf_device.h: train_compute_tiles)
    int32_t per;                // encoding scales per lane group of the saved h (nerf_layout.h: layer0_kernel_column)
    int32_t scales, enc_in, hidden, feat_tiles;
    int32_t distance;           // 1: the composited form (render_rays) — the distance route applies
    int64_t items;              // padded rays x chunks
};

// t_mean, t_var, r_var of one interval: the arithmetic of nerf_device.h: frustum
struct FrustumTerms {
    float t_mean, t_var, r_var;
};
__device__ __forceinline__ FrustumTerms frustum_terms(float t0, float t1, float base_radius_sq) {
#pragma clang fp contract(off)
    const float c415 = (float)(4.0 / 15.0), c512 = (float)(5.0 / 12.0);
    const float mu = (t0 + t1) / 2.0f;
    const float hw = (t1 - t0) / 2.0f;
    const float mu2 = mu * mu, hw2 = hw * hw, hw4 = hw2 * hw2;
    const float denom = 3.0f * mu2 + hw2;
    FrustumTerms f;
    f.t_mean = mu + (2.0f * mu * hw2) / denom;
    f.t_var = hw2 / 3.0f - c415 * ((hw4 * (12.0f * mu2 - hw2)) / (denom * denom));
    f.r_var = base_radius_sq * ((mu2 / 4.0f + c512 * hw2) - (c415 * hw4) / denom);
    return f;
}

__device__ __forceinline__ void add_at(float (&v)[3], int c, float x) {
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] += c == k ? x : 0.f;
}

__global__ __launch_bounds__(64 * kRayWaves) void nerf_ray_grad_kernel(const RayArgs ra) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* const w0l = (float*)smem;                                  // [16 ctiles][kW0Stride]
    const NerfHipRenderArgs& a = ra.a;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 15, g = lane >> 4;
    const int rows = 16 * ra.ctiles;
    for (int i = threadIdx.x; i < rows * kEncIn; i += 64 * kRayWaves) {
        const int n = i / kEncIn, f = i - n * kEncIn;
        w0l[n * kW0Stride + f] = n < ra.hidden && f < ra.enc_in ? ra.w0[(int64_t)n * ra.enc_in + f] : 0.f;
    }
    __syncthreads();
    const float* const ws = a.train_workspace;
    const int S3 = 3 * ra.scales;

    for (int64_t item = (int64_t)blockIdx.x * kRayWaves + wave; item < ra.items; item += (int64_t)gridDim.x * kRayWaves) {
        const int64_t slot = item / ra.chunks;
        const int c = (int)(item - slot * ra.chunks);
        const bool ray_ok = slot < a.n_rays;
        const int64_t local = ray_ok ? slot : a.n_rays - 1;
        const int s = 16 * c + j;
        const bool ok = ray_ok && s < ra.P;
        const int64_t sp = item * 16 + j;

        // ---- dL/dh^T [feature][sample] = W_0^T [feature][hidden] . dY_0^T [hidden][sample]: k-step (T, r) takes
        // hidden units 16 T + 4 g' + r (g' = 0..3); this lane gives B = dY_0[sample j][16 T + 4 g + r] (one f32x4 of
        // the tile-major row, nerf_device.h: tile_lane_word) and A = W_0[16 T + 4 g + r][16 ft + j].  Accumulator
        // ft, register q = dL/dh of feature 16 ft + 4 g + q (reference order) of sample j.
        f32x4 acc[kFeatTiles];
#pragma unroll
        for (int ft = 0; ft < kFeatTiles; ++ft) acc[ft] = f32x4{0.f, 0.f, 0.f, 0.f};
        const float* const dyt = ws + ra.L.dy[0] + item * 16 * ra.width + tile_lane_word(j, g);
        for (int T = 0; T < ra.ctiles; ++T) {
            const f32x4 b = *(const f32x4*)(dyt + T * kTileT);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float* const wrow = w0l + (16 * T + 4 * g + r) * kW0Stride + j;
#pragma unroll
                for (int ft = 0; ft < kFeatTiles; ++ft)
                    if (ft < ra.feat_tiles) acc[ft] = mfma4(wrow[16 * ft], b[r], acc[ft]);
            }
        }

        // ---- encoding backward: feature f = (part, scale k, coordinate cc), y = 2^(k-4) m_cc, v = 4^(k-4) cov_cc:
        //   dL/dm_cc += 2^(k-4) (g_sin h_cos - g_cos h_sin),   dL/dcov_cc += -1/2 4^(k-4) g h
        float dm[3] = {0.f, 0.f, 0.f}, dv[3] = {0.f, 0.f, 0.f};
        const float* const hrow = ws + ra.L.h + sp * kEncIn;
#pragma unroll
        for (int ft = 0; ft < kFeatTiles; ++ft) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int f = 16 * ft + 4 * g + q;
                if (f < ra.enc_in) {
                    const int part = f >= S3 ? 1 : 0;
                    const int rem = f - part * S3;
                    const int k = rem / 3, cc = rem - 3 * k;
                    const float scale = __builtin_ldexpf(1.0f, k - 4);
                    const float gv = acc[ft][q];
                    const float h_self = hrow[layer0_kernel_column(f, ra.scales, ra.per)];
                    const float h_other = hrow[layer0_kernel_column(part ? f - S3 : f + S3, ra.scales, ra.per)];
                    add_at(dm, cc, part ? -(scale * gv) * h_other : (scale * gv) * h_other);
                    add_at(dv, cc, -0.5f * (scale * scale) * gv * h_self);
                }
            }
        }
        // the four lane groups of a sample: one fixed association, the same bits in every lane
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            dm[k] += xor16(dm[k]);
            dm[k] += xor32(dm[k]);
            dv[k] += xor16(dv[k]);
            dv[k] += xor32(dv[k]);
        }

        // ---- frustum and distance: this sample's interval [t0, t1] and the next one's [t1, t2]
        float go[3] = {0.f, 0.f, 0.f}, gd[3] = {0.f, 0.f, 0.f};
        if (ok) {
            const Ray ray = load_ray(a, local);
            float posts[3];
            fencepost_run<3>(a, local, s, posts);
            const FrustumTerms ft0 = frustum_terms(posts[0], posts[1], a.base_radius_sq);
            const float dsq[3] = {ray.d[0] * ray.d[0], ray.d[1] * ray.d[1], ray.d[2] * ray.d[2]};
            const float mag_raw = (dsq[0] + dsq[1]) + dsq[2];
            const float mag = __builtin_fmaxf(mag_raw, 1e-10f);
            const float clamp_open = mag_raw >= 1e-10f ? 1.0f : 0.0f;     // torch.clamp(min=) passes the gradient there
            const float across = (dv[0] * dsq[0] + dv[1] * dsq[1]) + dv[2] * dsq[2];
            const float ring = ft0.r_var * clamp_open * across / (mag * mag);
            const float along = ft0.t_var - ft0.r_var / mag;
            float dmean[3] = {dm[0], dm[1], dm[2]};
            if (ra.d_mean != nullptr) {
                const float* dmp = ra.d_mean + ((int64_t)local * ra.P + s) * 3;
#pragma unroll
                for (int k = 0; k < 3; ++k) dmean[k] += dmp[k];
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                go[k] = dmean[k];
                gd[k] = ft0.t_mean * dmean[k] + 2.0f * ray.d[k] * (along * dv[k] + ring);
            }
            if (ra.distance && s < ra.P - 1) {
                // dist = |mean_{s+1} - mean_s| enters alpha as relu(sigma') dist: dL/d dist = dL/d sigma' sigma' / dist,
                // and d dist / d d = e (t_mean_{s+1} - t_mean_s) / dist; d dist / d o = 0
                const float* comp = ws + ra.L.comp + sp * 4;
                const float dist = comp[2], sig = comp[3];
                const float dsig = ws[ra.L.dy5 + sp * kOutPad];          // slot 0: density (nerf_layout.h: row_of_slot)
                if (dist > 0.f && sig > 0.f) {
                    const Gaussian ga = frustum(ray, posts[0], posts[1], a.base_radius_sq);
                    const Gaussian gb = frustum(ray, posts[1], posts[2], a.base_radius_sq);
                    const FrustumTerms ft1 = frustum_terms(posts[1], posts[2], a.base_radius_sq);
                    const float w = dsig * sig / (dist * dist) * (ft1.t_mean - ft0.t_mean);
#pragma unroll
                    for (int k = 0; k < 3; ++k) gd[k] += w * (gb.mean[k] - ga.mean[k]);
                }
            }
        }
        // ---- the chunk's 16 samples (lane group 0 holds them): a fixed DPP tree, lane 0 writes the partial
        float v[6];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            v[k] = g == 0 ? go[k] : 0.f;
            v[3 + k] = g == 0 ? gd[k] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) v[k] = row_sum(v[k]);
        if (lane == 0) {
            float* dst = ra.partial + item * kRayPartialFloats;
            *(f32x4*)dst = f32x4{v[0], v[1], v[2], v[3]};
            *(f32x4*)(dst + 4) = f32x4{v[4], v[5], 0.f, 0.f};
        }
    }
}

// per ray: the chunk partials in chunk order
__global__ __launch_bounds__(256) void nerf_ray_sum_kernel(const RayArgs ra) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ra.a.n_rays) return;
    float sum[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const float* p = ra.partial + i * ra.chunks * kRayPartialFloats;
    for (int c = 0; c < ra.chunks; ++c) {
#pragma unroll
        for (int k = 0; k < 6; ++k) sum[k] += p[c * kRayPartialFloats + k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (ra.d_rays_o != nullptr) ra.d_rays_o[i * 3 + k] = sum[k];
        if (ra.d_rays_d != nullptr) ra.d_rays_d[i * 3 + k] = sum[3 + k];
    }
}

int ray_chunks(int32_t num_samples) { return (num_samples - 1 + kSamplesPerWave - 1) / kSamplesPerWave; }

}  // namespace

extern "C" {

size_t nerf_hip_ray_backward_scratch_bytes(int64_t n_rays, int32_t num_samples) {
    if (n_rays <= 0 || num_samples < 2) return 0;
    return (size_t)((n_rays + 3) / 4 * 4) * ray_chunks(num_samples) * kRayPartialFloats * sizeof(float);
}

int nerf_hip_render_backward_rays(const NerfHipRayBackwardArgs* args, void* stream) {
    if (args == nullptr) return nerf_common::fail(NERF_HIP_EINVAL, "render_backward_rays: null args");
    const NerfHipBackwardArgs& b = args->bwd;
    const NerfHipRenderArgs& a = b.fwd;
    if (args->d_rays_o == nullptr && args->d_rays_d == nullptr)
        return nerf_common::fail(NERF_HIP_EINVAL, "render_backward_rays: neither d_rays_o nor d_rays_d is given");
    if (a.n_rays < 0 || a.num_samples < 2 || a.num_samples > 4096)
        return nerf_common::fail(NERF_HIP_EINVAL, "render_backward_rays: n_rays / num_samples out of range");
    if (!shape_ok(shape_of(a)))
        return nerf_common::fail(NERF_HIP_EUNSUPPORTED, "render_backward_rays: network shape out of range");
    if (a.n_rays > 0) {
        if (a.rays_o == nullptr || a.rays_d == nullptr)
            return nerf_common::fail(NERF_HIP_EINVAL, "render_backward_rays: rays must be explicit arrays");
        if (args->w0 == nullptr || args->ray_scratch == nullptr)
            return nerf_common::fail(NERF_HIP_EINVAL, "render_backward_rays: w0 or ray_scratch is null");
        if (b.scratch == nullptr || (b.d_rgb == nullptr && b.d_raw == nullptr))
            return nerf_common::fail(NERF_HIP_EINVAL, "render_backward_rays: scratch is null, or neither d_rgb nor d_raw is given");
        if (a.train_workspace == nullptr || a.packed == nullptr)
            return nerf_common::fail(NERF_HIP_EINVAL, "render_backward_rays: forward was not a training forward");
        if (b.d_seg != nullptr && a.seg == nullptr)
            return nerf_common::fail(NERF_HIP_EINVAL, "render_backward_rays: d_seg given but forward seg is null");
    }
    int rc = nerf_bwd::render_backward_launches(&b, stream, b.grad != nullptr);
    if (rc || a.n_rays == 0) return rc;
    hipStream_t st = (hipStream_t)stream;

    RayArgs ra;
    ra.a = a;
    ra.w0 = args->w0;
    ra.d_mean = args->d_mean;
    ra.partial = args->ray_scratch;
    ra.d_rays_o = args->d_rays_o;
    ra.d_rays_d = args->d_rays_d;
    const Shape sh = shape_of(a);
    const bool half = a.precision == NERF_HIP_PRECISION_F16X3;
    const int tt = train_tiles(sh.hidden), ct = train_compute_tiles(sh.hidden, half);
    ra.P = a.num_samples - 1;
    ra.chunks = ray_chunks(a.num_samples);
    ra.width = 16 * tt;
    ra.L = make_train_layout(a.n_rays, ra.chunks, ra.width);
    ra.ctiles = ct;
    ra.scales = sh.scales();
    ra.per = ct == 16 ? 4 : scales_per_group(ra.scales);    // the training forward's encode / encode_n
    ra.enc_in = sh.enc_in;
    ra.hidden = sh.hidden;
    ra.feat_tiles = (sh.enc_in + 15) / 16;
    ra.distance = b.d_raw == nullptr ? 1 : 0;
    ra.items = ra.L.mp / 16;

    int device = 0, cus = 0;
    rc = nerf_common::check_hip(hipGetDevice(&device), "hipGetDevice");
    if (rc) return rc;
    rc = nerf_common::check_hip(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device),
                                "hipDeviceGetAttribute");
    if (rc) return rc;
    const int lds = 16 * ct * kW0Stride * (int)sizeof(float);     // 100 KiB at 16 tiles
    static unsigned done = 0;
    rc = nerf_common::ensure_dynamic_lds((const void*)nerf_ray_grad_kernel, 16 * 16 * kW0Stride * (int)sizeof(float),
                                         device, &done);
    if (rc) return rc;
    int64_t grid = (ra.items + kRayWaves - 1) / kRayWaves;
    if (grid > cus) grid = cus;
    {
        nerf_common::TimedLaunch timed(st, NERF_HIP_TIMING_RAY_GRADIENT);
        hipLaunchKernelGGL(nerf_ray_grad_kernel, dim3((unsigned)grid), dim3(64 * kRayWaves), lds, st, ra);
        hipLaunchKernelGGL(nerf_ray_sum_kernel, dim3((unsigned)((a.n_rays + 255) / 256)), dim3(256), 0, st, ra);
    }
    return nerf_common::check_hip(hipGetLastError(), "render_backward_rays launch");
}

}  // extern "C"
