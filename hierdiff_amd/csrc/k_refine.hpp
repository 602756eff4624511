// The refine model (Node2Vec, models/model_refine.py of the reference): the parts around its E_GCL layers that are not dense GEMMs.
// Included through kernels.hpp.  Everything is exact fp32, deterministic (sums in a fixed order, no float atomics).
//
//   k_refine_embed        input gather: out[m][off_v + c] = Ev[v[m]][c], out[m][off_s + c] = Es[size[m]][c] - column blocks 0 and 2
//                         of the [M][3H] projection input (block 1 is written in place by the f_embedding GEMM).  An id outside
//                         its table writes zeros and raises *bad (the host checks it); it is never dereferenced.
//   k_refine_embed_bwd    dEv[id][c] = sum over rows m with v[m] == id of dout[m][off_v + c] (ascending m), same for dEs: one
//                         workgroup per table row, the ids staged through LDS 256 at a time.
//   k_sqdist / _bwd       ea[e] = |x[row e] - x[col e]|^2 on an hd_egcl_graph; dx[i] = sum_{row e = i} 2 dea[e] (x_i - x_col)
//                         - sum_{col e = i} 2 dea[e] (x_row - x_i), over the graph's CSR lists (edge order within a node fixed).
//   k_cand_xent / _bwd    the size-restricted softmax head: one wavefront per row over its candidate set (lanes stride the set,
//                         reductions with __shfl_xor over 64 lanes; any set size).  Forward: log-softmax over the set at the
//                         target, argmax == target, the top-k candidate ids (value descending, ties to the lower position in the
//                         set - torch.argmax's rule), k <= 16.  Backward: dlogits = dloss (softmax_set - onehot) on the set's
//                         columns and 0 elsewhere, assembled in LDS in chunks of columns so that every column is written once.
//                         Candidate ids outside [0, ncols) are never read (the forward reports them, err = 3).
#pragma once
#include "common.hpp"

#define HD_XENT_MAX_K 16
#define HD_XENT_CHUNK 1024

__global__ __launch_bounds__(256) void k_refine_embed(const long long* v, const long long* sz, int M, int H, int nv, int ns,
                                                      const float* Ev, const float* Es, float* out, int ldo, int off_v, int off_s,
                                                      int* bad) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)M * H) return;
    const int m = (int)(i / H), c = (int)(i % H);
    const long long a = v[m], b = sz[m];
    float ev = 0.0f, es = 0.0f;
    bool ok = true;
    if (a >= 0 && a < nv) ev = Ev[a * H + c]; else ok = false;
    if (b >= 0 && b < ns) es = Es[b * H + c]; else ok = false;
    if (!ok && bad) bad[0] = 1;
    out[(size_t)m * ldo + off_v + c] = ev;
    out[(size_t)m * ldo + off_s + c] = es;
}

__global__ __launch_bounds__(256) void k_refine_embed_bwd(const long long* v, const long long* sz, int M, int H, int nv,
                                                          const float* dout, int ldo, int off_v, int off_s, float* dEv,
                                                          float* dEs) {
    __shared__ long long ids[256];
    const bool is_v = (int)blockIdx.x < nv;
    const long long id = is_v ? (long long)blockIdx.x : (long long)blockIdx.x - nv;
    const long long* src = is_v ? v : sz;
    const int off = is_v ? off_v : off_s;
    float* dst = (is_v ? dEv : dEs) + id * H;
    for (int c0 = 0; c0 < H; c0 += 256) {
        const int c = c0 + (int)threadIdx.x;
        float acc = 0.0f;
        for (int m0 = 0; m0 < M; m0 += 256) {
            __syncthreads();
            const int m = m0 + (int)threadIdx.x;
            ids[threadIdx.x] = m < M ? src[m] : -1;
            __syncthreads();
            const int n = min(256, M - m0);
            if (c < H)
                for (int j = 0; j < n; ++j)
                    if (ids[j] == id) acc += dout[(size_t)(m0 + j) * ldo + off + c];
        }
        if (c < H) dst[c] = acc;
    }
}

__global__ __launch_bounds__(256) void k_sqdist(const int* row, const int* col, int E, const float* x, float* ea) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const float* a = x + (size_t)row[e] * 3;
    const float* b = x + (size_t)col[e] * 3;
    const float d0 = a[0] - b[0], d1 = a[1] - b[1], d2 = a[2] - b[2];
    ea[e] = d0 * d0 + d1 * d1 + d2 * d2;
}

__global__ __launch_bounds__(256) void k_sqdist_bwd(const int* row, const int* col, const int* rptr, const int* rrows,
                                                    const int* cptr, const int* crows, int M, const float* x, const float* dea,
                                                    float* dx) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const float xi0 = x[(size_t)i * 3], xi1 = x[(size_t)i * 3 + 1], xi2 = x[(size_t)i * 3 + 2];
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
    for (int k = rptr[i]; k < rptr[i + 1]; ++k) {          // i sends: d/dx_i of |x_i - x_col|^2
        const int e = rrows[k];
        const float* b = x + (size_t)col[e] * 3;
        const float g = 2.0f * dea[e];
        a0 += g * (xi0 - b[0]); a1 += g * (xi1 - b[1]); a2 += g * (xi2 - b[2]);
    }
    for (int k = cptr[i]; k < cptr[i + 1]; ++k) {          // i receives: d/dx_i of |x_row - x_i|^2
        const int e = crows[k];
        const float* a = x + (size_t)row[e] * 3;
        const float g = 2.0f * dea[e];
        a0 -= g * (a[0] - xi0); a1 -= g * (a[1] - xi1); a2 -= g * (a[2] - xi2);
    }
    dx[(size_t)i * 3] = a0; dx[(size_t)i * 3 + 1] = a1; dx[(size_t)i * 3 + 2] = a2;
}

struct CandXentArgs {
    const float* logits;    // [B][ld]
    const int* ids;         // candidate ids of all sets, set s at [off[s], off[s + 1])
    const int* off;         // [nsets + 1]
    const int* set;         // [B] set index per row
    const int* target;      // [B] target id per row
    float* logp;            // [B] forward: log-softmax over the set at the target (NaN if the target is not in the set)
    int* hit;               // [B] forward: argmax over the set == target
    int* topk;              // [B][k] forward: top-k ids (-1 past the set's size)
    int* err;               // forward: 1 a target outside its set, 2 a set index out of range, 3 a candidate id outside the
                            // columns (plain stores of a constant; zeroed by the caller)
    const float* dloss;     // [B] backward: d L / d (-logp[b]), the per-row cross-entropy's upstream gradient
    float* dlogits;         // [B][ld] backward (first ncols columns)
    int B, ld, ncols, nsets, k;
};

// (v, p) ordered by value descending, then position ascending: keep the better of two candidates
__device__ __forceinline__ void xent_better(float& v, int& p, float v2, int p2) {
    if (v2 > v || (v2 == v && p2 < p)) { v = v2; p = p2; }
}

__device__ __forceinline__ void xent_argmax_reduce(float& v, int& p) {
    for (int o = 32; o > 0; o >>= 1) {
        const float v2 = __shfl_xor(v, o);
        const int p2 = __shfl_xor(p, o);
        xent_better(v, p, v2, p2);
    }
}

__device__ __forceinline__ float xent_sum_reduce(float s) {
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);       // butterfly: every lane ends with the same bits
    return s;
}

__device__ __forceinline__ int xent_min_reduce(int t) {
    for (int o = 32; o > 0; o >>= 1) t = min(t, __shfl_xor(t, o));
    return t;
}

// a candidate's logit; an id outside the row reads as -inf and is counted in `bad`
__device__ __forceinline__ float xent_val(const float* row, int id, int ncols, int& bad) {
    if ((unsigned)id < (unsigned)ncols) return row[id];
    bad = 1;
    return -INFINITY;
}

// max, its position, log-sum-exp and the target's position over one row's set (every lane gets the same values)
__device__ __forceinline__ void xent_row_stats(const float* row, const int* cid, int n, int ncols, int tgt, int lane, float& mx,
                                               int& amax, float& lse, int& tpos, int& bad) {
    float bv = -INFINITY;
    int bp = 0x7fffffff, tp = 0x7fffffff;
    for (int j = lane; j < n; j += 64) {
        const int id = cid[j];
        xent_better(bv, bp, xent_val(row, id, ncols, bad), j);
        if (id == tgt) tp = min(tp, j);
    }
    xent_argmax_reduce(bv, bp);
    tp = xent_min_reduce(tp);
    float s = 0.0f;
    for (int j = lane; j < n; j += 64) s += expf(xent_val(row, cid[j], ncols, bad) - bv);
    s = xent_sum_reduce(s);
    mx = bv; amax = bp; lse = logf(s); tpos = tp;
}

__global__ __launch_bounds__(64) void k_cand_xent(CandXentArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= a.B) return;
    const int s = a.set[b];
    if (s < 0 || s >= a.nsets) {
        if (lane == 0) { a.err[0] = 2; a.logp[b] = NAN; a.hit[b] = 0; }
        for (int r = lane; r < a.k; r += 64) a.topk[(size_t)b * a.k + r] = -1;
        return;
    }
    const int beg = a.off[s], n = a.off[s + 1] - beg;
    const int* cid = a.ids + beg;
    const float* row = a.logits + (size_t)b * a.ld;
    float mx, lse;
    int amax, tp, bad = 0;
    xent_row_stats(row, cid, n, a.ncols, a.target[b], lane, mx, amax, lse, tp, bad);
    if (bad) a.err[0] = 3;
    if (lane == 0) {
        if (tp == 0x7fffffff) { a.err[0] = 1; a.logp[b] = NAN; a.hit[b] = 0; }
        else { a.logp[b] = (xent_val(row, cid[tp], a.ncols, bad) - mx) - lse; a.hit[b] = (amax == tp) ? 1 : 0; }
    }
    // top-k by repeated selection: the next entry is the best candidate strictly after the previous one in the (value desc,
    // position asc) order - no per-lane state, any set size
    float pv = INFINITY;
    int pp = -1;
    for (int r = 0; r < a.k; ++r) {
        if (r >= n) {
            if (lane == 0) a.topk[(size_t)b * a.k + r] = -1;
            continue;
        }
        float cv = -INFINITY;
        int cp = 0x7fffffff;
        for (int j = lane; j < n; j += 64) {
            const float val = xent_val(row, cid[j], a.ncols, bad);
            if (val < pv || (val == pv && j > pp)) xent_better(cv, cp, val, j);
        }
        xent_argmax_reduce(cv, cp);
        if (lane == 0) a.topk[(size_t)b * a.k + r] = cp < n ? cid[cp] : -1;
        pv = cv; pp = cp;
    }
}

__global__ __launch_bounds__(64) void k_cand_xent_bwd(CandXentArgs a) {
    __shared__ float buf[HD_XENT_CHUNK];
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= a.B) return;                                  // (one wavefront per workgroup: the barriers below are per row)
    const int s = a.set[b];
    const bool valid = s >= 0 && s < a.nsets;
    const int beg = valid ? a.off[s] : 0, n = valid ? a.off[s + 1] - beg : 0;
    const int* cid = a.ids + beg;
    const float* row = a.logits + (size_t)b * a.ld;
    float mx = 0.0f, lse = 0.0f;
    int amax = 0, tp = 0x7fffffff, bad = 0;
    if (valid) xent_row_stats(row, cid, n, a.ncols, a.target[b], lane, mx, amax, lse, tp, bad);
    const float g = a.dloss[b];
    float* drow = a.dlogits + (size_t)b * a.ld;
    for (int c0 = 0; c0 < a.ncols; c0 += HD_XENT_CHUNK) {
        for (int c = lane; c < HD_XENT_CHUNK; c += 64) buf[c] = 0.0f;
        __syncthreads();
        for (int j = lane; j < n; j += 64) {
            const int id = cid[j];
            if (id >= c0 && id < c0 + HD_XENT_CHUNK && id < a.ncols) {
                const float p = expf((row[id] - mx) - lse);
                buf[id - c0] = g * (j == tp ? p - 1.0f : p);
            }
        }
        __syncthreads();
        const int w = min(HD_XENT_CHUNK, a.ncols - c0);
        for (int c = lane; c < w; c += 64) drow[c0 + c] = buf[c];
        __syncthreads();
    }
}
