// Fragment-constrained sampling ("inpainting", hd_sample_loop_inpaint / hd_sample_path_inpaint): the replacement step behind every posterior step, the
// jump back of a resampling round and the fix-up behind the final decode.  No reference counterpart: the known fragments of a
// molecule are re-noised to the level of the current step and put in place of the generated rows (the replacement method of
// score-based models; with resamplings > 1 the RePaint form).  Included through kernels.hpp, after k_sampling.hpp.
//
// One workgroup (256 threads) per molecule, one thread per (node, component) as in k_post_step; every sum runs over the
// workgroup in the fixed order of block_sum4 (no atomics), so a molecule's bits depend on its own rows alone.  Exact fp32.
// Path position (the row of `coef`), draw and first sample id come from kernel arguments (plain launches) or from the path
// loop's device words (graph replay; k_path_state / k_path_advance in k_sampling.hpp keep the draws of all streams).
#pragma once
#include "k_sampling.hpp"

struct InpaintArgs {
    float* z;                   // [B][N][D] in place: z_gen -> z_s (replace), z_s -> z_t (jump)
    const uint8_t* nm;          // [B*N] node mask bytes
    const uint8_t* fixed;       // [B*N] fixed mask bytes (replace only); PARTS: "position known"
    const uint8_t* fixed_h;     // PARTS only: [B*N][D - 3] "feature channel known"
    const float* known;         // [B][N][D] normalised known values (replace only)
    const float* coef;          // [K][4] {alpha_s, sigma_s, alpha_t|s, sigma_t|s}, one row per path position (arrival level s)
    float row[4];               // the row by value when coef is null (hd_inpaint_replace)
    uint64_t seed, sample_base;
    uint32_t draw;
    int step;
    const uint32_t* draw_ptr;   // optional device-side draw (graph replay); overrides draw
    const int* step_ptr;        // optional device-side step index; overrides step
    const unsigned long long* base_ptr;   // optional device-side first global sample id; overrides sample_base
    int B, N, D;
};

// steps 2-3 of the algorithm (include/hierdiff_hip.h): z_kn = alpha_s known + sigma_s e_kn on the fixed rows, shifted so that the
// fixed block keeps the centre of gravity the generated rows had, then the masked mean removal of the plain step.
// A molecule without fixed nodes is left untouched.  Dynamic LDS = N * D floats.
// PARTS (hd_inpaint_parts, hd_inpaint_replace): an element is replaced when its own mask says so - a position component by
// `fixed`, a feature channel by `fixed_h` - and the shift and its count run over the position-fixed nodes alone.  A molecule
// without them has no frame: its known channels are written in place and the x part keeps its bits.  Same expressions in the same
// order as the whole-node form, so coinciding masks give its bits.
template <bool PARTS>
__global__ __launch_bounds__(256) void k_inpaint_replace(InpaintArgs a) {
    extern __shared__ float ip_s[];                // [N * D] blended z before the final re-centring
    __shared__ float red[4];
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    const int N = a.N, D = a.D, total = N * D;
    float nf = 0.f;
    for (int nn = tid; nn < N; nn += 256) nf += (a.fixed[b * N + nn] && a.nm[b * N + nn]) ? 1.f : 0.f;
    nf = block_sum4(nf, red, tid);
    if (!PARTS && nf == 0.f) return;               // uniform over the workgroup
    const uint64_t sid = (a.base_ptr ? (uint64_t)*a.base_ptr : a.sample_base) + (uint64_t)b;
    const uint32_t draw = a.draw_ptr ? *a.draw_ptr : a.draw;
    float alpha_s = a.row[0], sigma_s = a.row[1];
    if (a.coef) {
        const float* cf = a.coef + (size_t)(a.step_ptr ? *a.step_ptr : a.step) * 4;
        alpha_s = cf[0]; sigma_s = cf[1];
    }
    if (PARTS && nf == 0.f) {                      // uniform too: no frame, so no shift and no re-centring
        for (int e = tid; e < total; e += 256) {
            const int nn = e / D, c = e - nn * D;
            if (c < 3 || !a.nm[b * N + nn] || !a.fixed_h[((size_t)b * N + nn) * (D - 3) + (c - 3)]) continue;
            const size_t g = ((size_t)b * N + nn) * D + c;
            a.z[g] = alpha_s * a.known[g] + sigma_s * philox_normal(a.seed, sid, draw, (uint32_t)e);
        }
        return;
    }
    float sg[3] = {0.f, 0.f, 0.f}, sk[3] = {0.f, 0.f, 0.f}, cnt = 0.f;
    for (int e = tid; e < total; e += 256) {
        const int nn = e / D, c = e - nn * D;
        const bool valid = a.nm[b * N + nn] != 0;
        const bool fx = valid && a.fixed[b * N + nn] != 0;
        const size_t g = ((size_t)b * N + nn) * D + c;
        const float zg = a.z[g];
        const bool rep = (!PARTS || c < 3) ? fx : (valid && a.fixed_h[((size_t)b * N + nn) * (D - 3) + (c - 3)] != 0);
        float v = zg;
        if (rep) v = alpha_s * a.known[g] + sigma_s * philox_normal(a.seed, sid, draw, (uint32_t)e);
        ip_s[e] = v;
        if (c < 3) {
            if (fx) {
#pragma unroll
                for (int k = 0; k < 3; ++k) { if (c == k) { sg[k] += zg; sk[k] += v; } }
            }
            if (c == 0 && valid) cnt += 1.f;
        }
    }
    float shift[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) shift[k] = block_sum4(sg[k], red, tid) / nf - block_sum4(sk[k], red, tid) / nf;
    cnt = block_sum4(cnt, red, tid);
    float sv[3] = {0.f, 0.f, 0.f};
    for (int e = tid; e < total; e += 256) {       // each thread revisits its own elements: no barrier needed on ip_s
        const int nn = e / D, c = e - nn * D;
        if (c < 3) {
            float v = ip_s[e];
            if (a.nm[b * N + nn] && a.fixed[b * N + nn]) {
#pragma unroll
                for (int k = 0; k < 3; ++k) { if (c == k) v += shift[k]; }
                ip_s[e] = v;
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) { if (c == k) sv[k] += v; }
        }
    }
    float mean[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) mean[k] = block_sum4(sv[k], red, tid) / cnt;
    for (int e = tid; e < total; e += 256) {
        const int nn = e / D, c = e - nn * D;
        float v = ip_s[e];
        if (c < 3) {
            const float m = a.nm[b * N + nn] ? 1.f : 0.f;
#pragma unroll
            for (int k = 0; k < 3; ++k) { if (c == k) v -= mean[k] * m; }
        }
        a.z[((size_t)b * N + nn) * D + c] = v;
    }
}

// step 4: z_t = alpha_t|s z_s + sigma_t|s e_jump, e_jump the combined noise of the plain step (masked, x part mean-free over the
// molecule's valid nodes).  Dynamic LDS = N * D floats.
__global__ __launch_bounds__(256) void k_inpaint_jump(InpaintArgs a) {
    extern __shared__ float ip_s[];                // [N * D] masked raw normals
    __shared__ float red[4];
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    const int N = a.N, D = a.D, total = N * D;
    const uint64_t sid = (a.base_ptr ? (uint64_t)*a.base_ptr : a.sample_base) + (uint64_t)b;
    const uint32_t draw = a.draw_ptr ? *a.draw_ptr : a.draw;
    const float* cf = a.coef + (size_t)(a.step_ptr ? *a.step_ptr : a.step) * 4;
    const float alpha_ts = cf[2], sigma_ts = cf[3];
    float sn[3] = {0.f, 0.f, 0.f}, cnt = 0.f;
    for (int e = tid; e < total; e += 256) {
        const int nn = e / D, c = e - nn * D;
        const float m = a.nm[b * N + nn] ? 1.f : 0.f;
        const float z = philox_normal(a.seed, sid, draw, (uint32_t)e) * m;
        ip_s[e] = z;
        if (c < 3) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { if (c == k) sn[k] += z; }
            if (c == 0) cnt += m;
        }
    }
    float nmn[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) nmn[k] = block_sum4(sn[k], red, tid);
    cnt = block_sum4(cnt, red, tid);
    if (cnt == 0.f) return;                        // a molecule without valid nodes stays all zero
#pragma unroll
    for (int k = 0; k < 3; ++k) nmn[k] /= cnt;
    for (int e = tid; e < total; e += 256) {
        const int nn = e / D, c = e - nn * D;
        float z = ip_s[e];
        if (c < 3) {
            const float m = a.nm[b * N + nn] ? 1.f : 0.f;
#pragma unroll
            for (int k = 0; k < 3; ++k) { if (c == k) z -= nmn[k] * m; }
        }
        const size_t g = ((size_t)b * N + nn) * D + c;
        a.z[g] = alpha_ts * a.z[g] + sigma_ts * z;
    }
}

// Behind the final decode, in data units: h = h_known and x = x_known + (mean_fixed(x) - mean_fixed(x_known)) on the fixed rows - the
// returned fragments are a pure translation of the given ones.  One wavefront per molecule.
// PARTS (hd_inpaint_decode_fix_parts): x on the nodes of `fixed`, h per channel of `fixed_h`; a molecule without position-fixed
// nodes keeps its x.
struct InpaintFixArgs {
    const uint8_t* nm;
    const uint8_t* fixed;
    const uint8_t* fixed_h;     // PARTS only: [B*N][F]
    const float* x_known;       // [B][N][3]
    const float* h_known;       // [B][N][F]
    float* x;                   // [B][N][3]
    float* hfeat;               // [B][N][F]
    int B, N, F;
};

template <bool PARTS>
__global__ void k_inpaint_decode_fix(InpaintFixArgs a) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (b >= a.B) return;
    float sd[3] = {0.f, 0.f, 0.f}, sk[3] = {0.f, 0.f, 0.f}, nf = 0.f;
    for (int nn = lane; nn < a.N; nn += 64) {
        const size_t r = (size_t)b * a.N + nn;
        if (a.nm[r] && a.fixed[r]) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { sd[k] += a.x[r * 3 + k]; sk[k] += a.x_known[r * 3 + k]; }
            nf += 1.f;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        nf += __shfl_xor(nf, o);
#pragma unroll
        for (int k = 0; k < 3; ++k) { sd[k] += __shfl_xor(sd[k], o); sk[k] += __shfl_xor(sk[k], o); }
    }
    if (PARTS) {
        for (int nn = lane; nn < a.N; nn += 64) {
            const size_t r = (size_t)b * a.N + nn;
            if (!a.nm[r]) continue;
            for (int f = 0; f < a.F; ++f) { if (a.fixed_h[r * a.F + f]) a.hfeat[r * a.F + f] = a.h_known[r * a.F + f]; }
        }
    }
    if (nf == 0.f) return;
    float shift[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) shift[k] = sd[k] / nf - sk[k] / nf;
    for (int nn = lane; nn < a.N; nn += 64) {
        const size_t r = (size_t)b * a.N + nn;
        if (!(a.nm[r] && a.fixed[r])) continue;
#pragma unroll
        for (int k = 0; k < 3; ++k) a.x[r * 3 + k] = a.x_known[r * 3 + k] + shift[k];
        if (!PARTS) { for (int f = 0; f < a.F; ++f) a.hfeat[r * a.F + f] = a.h_known[r * a.F + f]; }
    }
}
