// Scoring molecules: every term of the variational bound inside the device loop (hd_set_nll_terms / hd_nll_terms / hd_nll_finish; no
// reference counterpart beyond the one-timestep estimator compute_loss, diffusion_qm9.py:530-673).  Included through kernels.hpp.
// Per term t of the uploaded list (position k, row {alpha_t, sigma_t, w_t, 0}):
//   (a) k_nll_zt    eps_t = combined noise (masked, x part mean-free over the valid nodes), z_t = alpha_t xh + sigma_t eps_t
//       [network call at tau[t] on z_t -> eps^_t]
//   (b) k_nll_err   e_t = sum_{nodes, columns} (eps_t - eps^_t)^2,  acc[b] += w_t e_t          (acc: double, one thread per molecule)
// and once per score
//   (c) k_nll_finish  nll = kl_prior + (T / K) fp32(acc) + neg_log_constants + L_0 - delta_log_px  from (xh, z_0, eps_0, eps^_0).
// One workgroup (256 threads) per molecule, as k_post_step: each normal is produced once and kept in LDS for the mean removal; sums
// over a molecule's nodes run in a fixed order (strided per thread, then vlb_block_sum of k_loss.hpp); no atomics.  Draw layout of
// the generator at hd_noise (include/hierdiff_hip.h): term t draws at `t`, eps_0 at 0.
#pragma once
#include "common.hpp"
#include "k_sampling.hpp"
#include "k_loss.hpp"

struct NllZtArgs {
    const float* xh;      // [B][N][D] normalised data
    const uint8_t* nm;    // [B*N] node mask bytes
    float* eps;           // [B][N][D] out: eps_t
    float* zt;            // [B][N][D] out: z_t
    const float* coef;    // [K][4] term rows {alpha_t, sigma_t, w_t, 0}, or null: alpha / sigma below (the t = 0 draw of the finish)
    NoiseSrc noise;
    const int* step_ptr;                  // optional device-side term position (graph replay); otherwise `k`
    const uint32_t* draw_ptr;             // optional device-side draw counter (graph replay); overrides noise.draw
    const unsigned long long* base_ptr;   // optional device-side first global sample id (graph replay)
    float alpha, sigma;
    int k, raw_k0;        // raw_k0: injected normals of position k start at row block k - raw_k0
    int B, N, D, F;
};

__global__ __launch_bounds__(256) void k_nll_zt(NllZtArgs a) {
    extern __shared__ float nll_nz[];              // [N * D] masked raw normals
    __shared__ float red[4 * 4];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int N = a.N, D = a.D, total = N * D;
    const int k = a.step_ptr ? *a.step_ptr : a.k;
    NoiseSrc ns = a.noise;
    if (a.base_ptr) ns.sample_base = *a.base_ptr;
    if (a.draw_ptr) ns.draw = *a.draw_ptr;
    if (ns.raw_x) {
        const size_t off = (size_t)(k - a.raw_k0) * ns.rows * N;
        ns.raw_x += off * 3;
        ns.raw_h += off * a.F;
    }
    const float alpha = a.coef ? a.coef[(size_t)k * 4] : a.alpha;
    const float sigma = a.coef ? a.coef[(size_t)k * 4 + 1] : a.sigma;
    float v[4] = {0.f, 0.f, 0.f, 0.f};             // masked sums of the x noise per component, node count
    for (int e = tid; e < total; e += 256) {
        const int nn = e / D, c = e - nn * D;
        const float m = a.nm[b * N + nn] ? 1.f : 0.f;
        const float z = raw_noise(ns, b, nn, c, N, a.F) * m;
        nll_nz[e] = z;
#pragma unroll
        for (int j = 0; j < 3; ++j) { if (c == j) v[j] += z; }
        if (c == 0) v[3] += m;
    }
    vlb_block_sum<4>(v, red);
    const float mean[3] = {v[0] / v[3], v[1] / v[3], v[2] / v[3]};
    const size_t base = (size_t)b * total;
    for (int e = tid; e < total; e += 256) {
        const int nn = e / D, c = e - nn * D;
        float z = nll_nz[e];
        if (c < 3) {
            const float m = a.nm[b * N + nn] ? 1.f : 0.f;
#pragma unroll
            for (int j = 0; j < 3; ++j) { if (c == j) z -= mean[j] * m; }
        }
        a.eps[base + e] = z;
        a.zt[base + e] = alpha * a.xh[base + e] + sigma * z;
    }
}

struct NllErrArgs {
    const float* eps;     // [B][N][D] eps_t
    const float* net;     // [B][N][D] network output
    const float* coef;    // [K][4]
    double* acc;          // [B]
    float* err;           // [K][B] or null: e_t of position k at row k
    const int* step_ptr;
    int k, B, ND;
};

__global__ __launch_bounds__(256) void k_nll_err(NllErrArgs a) {
    __shared__ float red[4];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int k = a.step_ptr ? *a.step_ptr : a.k;
    const size_t base = (size_t)b * a.ND;
    float v[1] = {0.f};
    for (int i = tid; i < a.ND; i += 256) {
        const float r = a.eps[base + i] - a.net[base + i];
        v[0] += r * r;
    }
    vlb_block_sum<1>(v, red);
    if (tid == 0) {
        a.acc[b] += (double)a.coef[(size_t)k * 4 + 2] * (double)v[0];
        if (a.err) a.err[(size_t)k * a.B + b] = v[0];
    }
}

// The t-independent rest of compute_loss(t0_always = True) and the sum: the expressions of k_vlb (k_loss.hpp) with (z_t, g_t, eps,
// net) = (z_0, g_0, eps_0, eps^_0).
struct NllFinishArgs {
    const float* net;     // [B][N][D] eps^_0
    const float* z0;      // [B][N][D]
    const float* xh;      // [B][N][D]
    const float* eps;     // [B][N][D] eps_0
    const uint8_t* nm;    // [B*N]
    const double* acc;    // [B] sum_t w_t e_t
    float* nll;           // [B]
    float g0, gT, scale;  // gamma at 0 and 1; scale = T / K
    float nv2, nb2, log_nv0;
    int B, N, D, int_nf, cont_nf;
};

__global__ __launch_bounds__(256) void k_nll_finish(NllFinishArgs a) {
    __shared__ float red[4 * 4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int N = a.N, D = a.D, nd = 3;
    const size_t base = (size_t)b * N * D;
    const float sigma_0 = sqrtf(vlb_sigmoid(a.g0));
    const float inv_s0 = 1.0f / (sigma_0 * a.nv2);
    float v[4] = {0.f, 0.f, 0.f, 0.f};             // {Ex + Eh, sum xh^2 (h masked), n, log_int}
    for (int idx = tid; idx < N * D; idx += 256) {
        const int n = idx / D, d = idx - n * D;
        const float m = a.nm[b * N + n] ? 1.f : 0.f;
        const float e = a.eps[base + idx], x = a.xh[base + idx];
        if (d < nd) { const float r = e - a.net[base + idx]; v[0] += r * r; }
        v[1] += (d < nd) ? x * x : m * x * x;
        if (d == 0) v[2] += m;
        if (d >= nd + a.int_nf && d < nd + a.int_nf + a.cont_nf) {                 // eps[n][3 + int + c] against net[n][0]
            const float rc = e - a.net[base + (size_t)n * D];
            v[0] += rc * rc;
        }
        if (d >= nd && d < nd + a.int_nf) {
            const float hint = rintf(x * a.nv2 + a.nb2);
            const float c = hint - (a.z0[base + idx] * a.nv2 + a.nb2);
            v[3] += m * logf(vlb_cdf((c + 0.5f) * inv_s0) - vlb_cdf((c - 0.5f) * inv_s0) + 1e-10f);
        }
    }
    vlb_block_sum<4>(v, red);
    if (tid != 0) return;
    const float S = v[1], n = v[2];
    const float F = (float)(D - nd), dsub = (n - 1.0f) * nd;
    const float L0 = 0.5f * v[0] - v[3];
    const float uT = vlb_sigmoid(a.gT), aT2 = vlb_sigmoid(-a.gT);
    const float K = (n * F + dsub) * (-0.5f * logf(uT) + 0.5f * uT - 0.5f) + 0.5f * aT2 * S;
    const float C0 = (dsub + n * F) * (0.5f * a.g0 + 0.91893853320467274f);
    const float delta = -dsub * a.log_nv0;
    a.nll[b] = K + a.scale * (float)a.acc[b] + C0 + L0 - delta;
}

// graph replay: the term position lives in `step`; network time tau[t_idx[k]] and draw t_idx[k] follow it (k_path_advance's scheme).
// Behind the last term the words keep the values of k = K - 1; nothing reads them.
struct NllWords {
    int* step;
    uint32_t* draw;
    float* t_cur;
    unsigned long long* base;
    const float* tau;     // [T + 1]
    const int* t_idx;     // [K]
    int K;
};

HD_DEVINL void nll_words_set(const NllWords& w, int k) {
    const int t = w.t_idx[k < w.K ? k : w.K - 1];
    *w.step = k; *w.draw = (uint32_t)t; *w.t_cur = w.tau[t];
}

__global__ void k_nll_state(NllWords w, int k0, unsigned long long b0) {
    *w.base = b0;
    nll_words_set(w, k0);
}

__global__ void k_nll_advance(NllWords w) { nll_words_set(w, *w.step + 1); }
