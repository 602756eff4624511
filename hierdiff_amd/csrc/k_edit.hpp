// Editing given molecules (hd_diffuse / hd_set_path_up / hd_slerp; no reference counterpart).  Included through kernels.hpp.
//   k_diffuse   z = alpha xh + sigma eps, eps = combined noise (masked, x part mean-free over the valid nodes): the start state of a
//               partial reverse chain (SDEdit-style variations) and, with sigma == 0, of an inversion (z_0 = alpha_0 xh, no normal is
//               generated or read).
//   k_slerp     spherical interpolation of two latents per molecule, all frames of up to SLERP_CHUNK weights in one launch.
// The inversion itself needs no kernel of its own: an ascending path is rows {a, b, 0, 0} of k_post_step<1> (k_sampling.hpp).
// One workgroup (256 threads) per molecule as k_nll_zt: each normal is produced once and kept in LDS for the mean removal; sums over
// a molecule's nodes run in a fixed order; no atomics; exact fp32 (k_slerp: sums and angle in double).
#pragma once
#include "common.hpp"
#include "k_sampling.hpp"

struct DiffuseArgs {
    const float* xh;      // [B][N][D] normalised data
    const uint8_t* nm;    // [B*N] node mask bytes
    float* z;             // [B][N][D] out
    NoiseSrc noise;
    const uint32_t* draw_ptr;             // optional device-side draw counter; overrides noise.draw
    const unsigned long long* base_ptr;   // optional device-side first global sample id; overrides noise.sample_base
    float alpha, sigma;
    int B, N, D, F;
};

// The x-noise means are summed in k_noise's order (lane l adds nodes l, l + 64, .., then the xor butterfly; every wavefront repeats it
// on the LDS copy), not per thread and vlb_block_sum as k_nll_zt does: eps is then hd_noise's tensor at the same (seed, id, draw) bit
// for bit, so a start state at draw 0 holds exactly the normals plain sampling would have used for z_T.
__global__ __launch_bounds__(256) void k_diffuse(DiffuseArgs a) {
    extern __shared__ float df_nz[];               // [N * D] masked raw normals
    const int tid = threadIdx.x, b = blockIdx.x, lane = tid & 63;
    const int N = a.N, D = a.D, total = N * D;
    const size_t base = (size_t)b * total;
    if (a.sigma == 0.f) {                          // uniform over the grid
        for (int e = tid; e < total; e += 256) a.z[base + e] = a.alpha * a.xh[base + e];
        return;
    }
    NoiseSrc ns = a.noise;
    if (a.base_ptr) ns.sample_base = *a.base_ptr;
    if (a.draw_ptr) ns.draw = *a.draw_ptr;
    for (int e = tid; e < total; e += 256) {
        const int nn = e / D, c = e - nn * D;
        const float m = a.nm[b * N + nn] ? 1.f : 0.f;
        df_nz[e] = raw_noise(ns, b, nn, c, N, a.F) * m;
    }
    __syncthreads();
    float v[4] = {0.f, 0.f, 0.f, 0.f};             // masked sums of the x noise per component, node count
    for (int nn = lane; nn < N; nn += 64) {
#pragma unroll
        for (int j = 0; j < 3; ++j) v[j] += df_nz[nn * D + j];
        v[3] += a.nm[b * N + nn] ? 1.f : 0.f;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] += __shfl_xor(v[j], o);
    }
    float mean[3] = {0.f, 0.f, 0.f};
    if (v[3] > 0.f) { mean[0] = v[0] / v[3]; mean[1] = v[1] / v[3]; mean[2] = v[2] / v[3]; }
    for (int e = tid; e < total; e += 256) {
        const int nn = e / D, c = e - nn * D;
        float z = df_nz[e];
        if (c < 3) {
            const float m = a.nm[b * N + nn] ? 1.f : 0.f;
#pragma unroll
            for (int j = 0; j < 3; ++j) { if (c == j) z -= mean[j] * m; }
        }
        a.z[base + e] = a.alpha * a.xh[base + e] + a.sigma * z;
    }
}

// out[l] = (sin((1 - lam_l) theta) za + sin(lam_l theta) zb) / sin theta per molecule, theta the angle between the two latents over the
// valid entries; dot and squared norms accumulate in double (strided per thread, then the fixed tree below).  sin theta < SLERP_EPS
// (parallel or antiparallel latents, or a zero one): the linear form (1 - lam) za + lam zb.  lam == 0 / lam == 1 copy za / zb.
// No re-centring: a linear combination of mean-free x parts is mean-free, and the endpoints stay exact.
#define SLERP_CHUNK 64
#define SLERP_EPS 1e-6

struct SlerpArgs {
    const float* za;      // [B][N][D]
    const float* zb;      // [B][N][D]
    const uint8_t* nm;    // [B*N]
    float* out;           // [L][B][N][D]; this launch writes frames l0 .. l0 + n - 1
    float lam[SLERP_CHUNK];
    int l0, n;
    int B, N, D;
};

__global__ __launch_bounds__(256) void k_slerp(SlerpArgs a) {
    __shared__ double red[4 * 3];
    __shared__ float w[2];
    const int tid = threadIdx.x, b = blockIdx.x, li = blockIdx.y;
    const int lane = tid & 63, wave = tid >> 6;
    const int N = a.N, D = a.D, total = N * D;
    const size_t base = (size_t)b * total;
    const float lam = a.lam[li];
    float* out = a.out + ((size_t)(a.l0 + li) * a.B + b) * total;
    if (lam == 0.f || lam == 1.f) {                // uniform over the workgroup
        const float* src = lam == 0.f ? a.za : a.zb;
        for (int e = tid; e < total; e += 256) out[e] = a.nm[b * N + e / D] ? src[base + e] : 0.f;
        return;
    }
    double v[3] = {0.0, 0.0, 0.0};                 // dot, |za|^2, |zb|^2
    for (int e = tid; e < total; e += 256) {
        if (!a.nm[b * N + e / D]) continue;
        const double x = (double)a.za[base + e], y = (double)a.zb[base + e];
        v[0] += x * y; v[1] += x * x; v[2] += y * y;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o);
    if (lane == 0) { red[wave * 3] = v[0]; red[wave * 3 + 1] = v[1]; red[wave * 3 + 2] = v[2]; }
    __syncthreads();
    if (tid == 0) {
        const double dot = (red[0] + red[3]) + (red[6] + red[9]);
        const double na = (red[1] + red[4]) + (red[7] + red[10]), nb = (red[2] + red[5]) + (red[8] + red[11]);
        const double den = sqrt(na) * sqrt(nb);
        double wa = 1.0 - (double)lam, wb = (double)lam;
        if (den > 0.0) {
            const double c = fmin(fmax(dot / den, -1.0), 1.0);
            const double theta = acos(c), st = sin(theta);
            if (st >= SLERP_EPS) { wa = sin((1.0 - (double)lam) * theta) / st; wb = sin((double)lam * theta) / st; }
        }
        w[0] = (float)wa; w[1] = (float)wb;
    }
    __syncthreads();
    const float wa = w[0], wb = w[1];
    for (int e = tid; e < total; e += 256)
        out[e] = a.nm[b * N + e / D] ? wa * a.za[base + e] + wb * a.zb[base + e] : 0.f;
}
