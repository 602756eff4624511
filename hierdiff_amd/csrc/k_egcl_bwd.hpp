// Stage-2 layer E_GCL (/root/reference/models/egnn/gcl.py:9-205), BACKWARD: the row-wise kernels between the dense
// contractions of hd_egcl_backward (hierdiff_hip.hip).  Included through kernels.hpp, after k_egcl.hpp and k_tgemm.hpp.
//
// Every dense product of the backward (dX = dY W, dW = dY^T X over node or edge rows, split-K in slab order) runs on the
// library's exact-fp32 training GEMM (k_tgemm); what is left between them is element-wise or a per-edge dot product:
//   k_egcl_bnode_in    node inputs of the node model's backward: X = [h | agg], dout = dh_out * node_mask, dxs = dx_out * node_mask
//   k_egcl_bmask       dL/d(edge_mlp.2 output) = dedge_attr_out * edge_mask
//   k_egcl_bcoord      coordinate head: through tanh * coords_range, the edge mask and cdiff's direction; dpc = dphi w_c2 SiLU'(pc)
//   k_egcl_bgate       dagg[col] gathered into the message gradient, attention gate + edge mask, SiLU' of mes_mlp.2
//   k_egcl_bgeo        the per-edge distance: d(radial) from the message input (radial or 1 / radial^2), edge_mlp.0's radial
//                      column and cdiff = diff / (sqrt(radial + 1e-8) + 1) -> d(diff)
//   k_egcl_bnode_out   dh (residual, node model input, A / B halves of mes_mlp.0, the context quirk) and dx as CSR sums over the
//                      sending (row) and receiving (col) index in ascending edge order - no atomics: the gradient is deterministic
// One wavefront per edge row for the kernels with a dot product over the H features (H <= 256: one float4 per lane).
#pragma once
#include "common.hpp"

struct EgclBNodeInArgs {
    const float* h;         // [M][H+ctx]
    const float* agg;       // [M][H] (saved by hd_egcl_forward_train)
    const float* dh_out;    // [M][H+ctx] or NULL
    const float* dx_out;    // [M][3] or NULL
    const float* nmask;     // [M] or NULL
    float* X;               // [M][2H] = [h[:, :H] | agg]
    float* dout;            // [M][H]  = dh_out[:, :H] * node_mask
    float* dxs;             // [M][4]  = dx_out * node_mask (4th = 0)
    int M, H, ctx;
};

__global__ void k_egcl_bnode_in(EgclBNodeInArgs a) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int H2 = 2 * a.H, W = a.H + a.ctx;
    const int i = (int)(idx / H2), k = (int)(idx - (long long)i * H2);
    if (i >= a.M) return;
    const float m = a.nmask ? a.nmask[i] : 1.0f;
    a.X[(size_t)i * H2 + k] = (k < a.H) ? a.h[(size_t)i * W + k] : a.agg[(size_t)i * a.H + k - a.H];
    if (k < a.H) a.dout[(size_t)i * a.H + k] = a.dh_out ? a.dh_out[(size_t)i * W + k] * m : 0.0f;
    if (k < 4) a.dxs[(size_t)i * 4 + k] = (k < 3 && a.dx_out) ? a.dx_out[(size_t)i * 3 + k] * m : 0.0f;
}

// out[e][:] = in[e][:] * edge_mask[e]  (in NULL: zeros)
struct EgclBMaskArgs {
    const float* in;        // [E][H] or NULL
    const float* emask;     // [E] or NULL
    float* out;             // [E][H]
    int E, H;
};

__global__ void k_egcl_bmask(EgclBMaskArgs a) {
    const int q = a.H >> 2;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int e = (int)(idx / q), c4 = (int)(idx - (long long)e * q);
    if (e >= a.E) return;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (a.in) v = *reinterpret_cast<const f32x4*>(a.in + (size_t)e * a.H + 4 * c4) * (a.emask ? a.emask[e] : 1.0f);
    *reinterpret_cast<f32x4*>(a.out + (size_t)e * a.H + 4 * c4) = v;
}

HD_DEVINL float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Coordinate head (gcl.py:130-152): phi = C1 . w_c2,  sc = (tanh(phi) coords_range | phi) * m,  trans = cdiff * sc,
// x_out[col] += trans.  Given dtrans = dxs[col]:  dsc = dtrans . cdiff,  dcdiff = dtrans * sc (to escal, finished by
// k_egcl_bgeo),  dphi = dsc * m * (coords_range (1 - tanh^2) | 1),  dpc = dphi w_c2 SiLU'(pc);  dphi also to sc4[e].y
// (the operand of d(w_c2) = dphi^T C1).
struct EgclBCoordArgs {
    const float* C1;        // [E][H] = SiLU(pc)
    const float* pc;        // [E][H] pre-activation of coord_mlp.0
    const float* wc2;       // [H]
    const float* geo;       // [E][4] = {cdiff, radial}
    const int* col;
    const float* dxs;       // [M][4]
    const float* emask;     // [E] or NULL
    float* dpc;             // [E][H]
    float* escal;           // [E][4] <- {dcdiff, 0}
    float* sc4;             // [E][4], .y <- dphi
    float range;
    int E, H, use_tanh;
};

__global__ void k_egcl_bcoord(EgclBCoordArgs a) {
    const int lane = threadIdx.x & 63;
    const int e = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (e >= a.E) return;
    const int k = lane * 4;
    const bool on = k < a.H;
    f32x4 c1 = {0.f, 0.f, 0.f, 0.f}, w = {0.f, 0.f, 0.f, 0.f};
    if (on) {
        c1 = *reinterpret_cast<const f32x4*>(a.C1 + (size_t)e * a.H + k);
        w = *reinterpret_cast<const f32x4*>(a.wc2 + k);
    }
    float dot = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) dot = __builtin_fmaf(c1[j], w[j], dot);
    const float phi = wave_sum(dot);
    const float m = a.emask ? a.emask[e] : 1.0f;
    const float th = tanhf(phi);
    const float sc = (a.use_tanh ? th * a.range : phi) * m;
    const f32x4 g = *reinterpret_cast<const f32x4*>(a.geo + (size_t)e * 4);
    const f32x4 dt = *reinterpret_cast<const f32x4*>(a.dxs + (size_t)a.col[e] * 4);
    const float dsc = dt[0] * g[0] + dt[1] * g[1] + dt[2] * g[2];
    const float dphi = dsc * m * (a.use_tanh ? a.range * (1.0f - th * th) : 1.0f);
    if (on) {
        const f32x4 p = *reinterpret_cast<const f32x4*>(a.pc + (size_t)e * a.H + k);
        f32x4 d;
#pragma unroll
        for (int j = 0; j < 4; ++j) d[j] = dphi * w[j] * dsilu_f(p[j]);
        *reinterpret_cast<f32x4*>(a.dpc + (size_t)e * a.H + k) = d;
    }
    if (lane == 0) {
        *reinterpret_cast<f32x4*>(a.escal + (size_t)e * 4) = f32x4{dt[0] * sc, dt[1] * sc, dt[2] * sc, 0.f};
        a.sc4[(size_t)e * 4 + 1] = dphi;
    }
}

// Message gate (gcl.py:99-107): ef = M1 * s * m with M1 = SiLU(pre2), s = sigmoid(M1 . wa + ba) (attention) or 1.
//   def   = defp[e] + dagg[col[e]]                           (edge-update / coordinate contributions + the node sum's gather)
//   t     = (def . M1) m s (1 - s)                           -> sc4[e].x  (d(wa) = t^T M1, d(ba) = sum t)
//   dpre2 = (def s m + t wa) SiLU'(pre2)
struct EgclBGateArgs {
    const float* defp;      // [E][H] or NULL
    const float* dagg;      // [M][ld_dagg]
    const int* col;
    const float* pre2;      // [E][H]
    const float* wa;        // [H]
    const float* ba;        // [1]
    const float* emask;     // [E] or NULL
    float* dpre2;           // [E][H]
    float* M1;              // [E][H] (attention only: the operand of d(wa))
    float* sc4;             // [E][4], .x <- t
    int E, H, ld_dagg, attention;
};

__global__ void k_egcl_bgate(EgclBGateArgs a) {
    const int lane = threadIdx.x & 63;
    const int e = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (e >= a.E) return;
    const int k = lane * 4;
    const bool on = k < a.H;
    f32x4 d = {0.f, 0.f, 0.f, 0.f}, p = {0.f, 0.f, 0.f, 0.f}, mm = {0.f, 0.f, 0.f, 0.f}, w = {0.f, 0.f, 0.f, 0.f};
    if (on) {
        d = *reinterpret_cast<const f32x4*>(a.dagg + (size_t)a.col[e] * a.ld_dagg + k);
        if (a.defp) d += *reinterpret_cast<const f32x4*>(a.defp + (size_t)e * a.H + k);
        p = *reinterpret_cast<const f32x4*>(a.pre2 + (size_t)e * a.H + k);
#pragma unroll
        for (int j = 0; j < 4; ++j) mm[j] = silu_f(p[j]);
        if (a.attention) w = *reinterpret_cast<const f32x4*>(a.wa + k);
    }
    const float m = a.emask ? a.emask[e] : 1.0f;
    float s = 1.0f, t = 0.0f;
    if (a.attention) {
        float d1 = 0.f, d2 = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) { d1 = __builtin_fmaf(mm[j], w[j], d1); d2 = __builtin_fmaf(d[j], mm[j], d2); }
        d1 = wave_sum(d1);
        d2 = wave_sum(d2);
        s = sigmoid_f(d1 + a.ba[0]);
        t = d2 * m * s * (1.0f - s);
    }
    if (on) {
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = __builtin_fmaf(d[j], s * m, t * w[j]) * dsilu_f(p[j]);
        *reinterpret_cast<f32x4*>(a.dpre2 + (size_t)e * a.H + k) = o;
        if (a.attention) *reinterpret_cast<f32x4*>(a.M1 + (size_t)e * a.H + k) = mm;
    }
    if (lane == 0) a.sc4[(size_t)e * 4] = t;
}

// Per-edge distance (gcl.py:198-205, :91-116).  diff = x[row] - x[col], radial = |diff|^2, rin = radial or 1 / radial^2 (geo):
//   d(radial) = (dpre1 . w_r) d(rin)/d(radial) + (dpe . w_er) + (dcdiff . diff) d(inv)/d(radial)
//   d(diff)   = dcdiff inv + 2 d(radial) diff,      inv = 1 / (sqrt(radial + 1e-8) + 1)
// -> escal[e] = {d(diff), 0};  rin -> sc4[e].z (the operand of d(w_r) = dpre1^T rin).
struct EgclBGeoArgs {
    const float* dpre1;     // [E][H]
    const float* w_r;       // w_r[k * ld_wr]: the radial column of mes_mlp.0
    const float* dpe;       // [E][H] or NULL (no edge update)
    const float* w_er;      // w_er[k * ld_wer]: the radial column of edge_mlp.0
    const float* x;         // [M][3]
    const int* row;
    const int* col;
    float* escal;           // [E][4]: in {dcdiff, 0} (coord_in), out {d(diff), 0}
    float* sc4;             // [E][4], .z <- rin
    int E, H, ld_wr, ld_wer, geo_mode, coord_in;
};

__global__ void k_egcl_bgeo(EgclBGeoArgs a) {
    const int lane = threadIdx.x & 63;
    const int e = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (e >= a.E) return;
    float d1 = 0.f, d2 = 0.f;
    for (int k = lane; k < a.H; k += 64) {
        d1 = __builtin_fmaf(a.dpre1[(size_t)e * a.H + k], a.w_r[(size_t)k * a.ld_wr], d1);
        if (a.dpe) d2 = __builtin_fmaf(a.dpe[(size_t)e * a.H + k], a.w_er[(size_t)k * a.ld_wer], d2);
    }
    d1 = wave_sum(d1);
    d2 = wave_sum(d2);
    if (lane != 0) return;
    const int r = a.row[e], c = a.col[e];
    const float dx = a.x[(size_t)r * 3] - a.x[(size_t)c * 3], dy = a.x[(size_t)r * 3 + 1] - a.x[(size_t)c * 3 + 1],
                dz = a.x[(size_t)r * 3 + 2] - a.x[(size_t)c * 3 + 2];
    const float radial = dx * dx + dy * dy + dz * dz;
    float drad = (a.geo_mode ? d1 * (-2.0f / (radial * radial * radial)) : d1) + d2;
    f32x4 dd = {0.f, 0.f, 0.f, 0.f};
    if (a.coord_in) {
        const f32x4 dcd = *reinterpret_cast<const f32x4*>(a.escal + (size_t)e * 4);
        const float sq = sqrtf(radial + 1e-8f);
        const float inv = 1.0f / (sq + 1.0f);
        drad += (dcd[0] * dx + dcd[1] * dy + dcd[2] * dz) * (-inv * inv / (2.0f * sq));
        dd = f32x4{dcd[0] * inv, dcd[1] * inv, dcd[2] * inv, 0.f};
    }
    dd[0] = __builtin_fmaf(2.0f * drad, dx, dd[0]);
    dd[1] = __builtin_fmaf(2.0f * drad, dy, dd[1]);
    dd[2] = __builtin_fmaf(2.0f * drad, dz, dd[2]);
    *reinterpret_cast<f32x4*>(a.escal + (size_t)e * 4) = dd;
    a.sc4[(size_t)e * 4 + 2] = a.geo_mode ? 1.0f / (radial * radial) : radial;
}

// dh[i][k], k < H:  (recurrent: dout) + dX[i][k] (node_mlp.0, h half) + T2[i][k] (dA W1a + dB W1b), and for the last ctx hidden
//                   columns (the context the reference slices from the already truncated h, gcl.py:162-164): + Tc (dA W_c) +
//                   dh_out[i][H + .] * node_mask (the context columns of the output);   k >= H: 0 (columns the layer drops)
// dx[i] = dxs[i] + sum_{e: row = i} d(diff)[e] - sum_{e: col = i} d(diff)[e], both lists in ascending edge order.
struct EgclBNodeOutArgs {
    const float* dout;      // [M][H]
    const float* dX;        // [M][2H]
    const float* T2;        // [M][H] or NULL
    const float* Tc;        // [M][ctx] or NULL
    const float* dh_out;    // [M][H+ctx] or NULL
    const float* nmask;     // [M] or NULL
    const float* dxs;       // [M][4]
    const float* escal;     // [E][4]
    const int* rptr; const int* rrows;
    const int* cptr; const int* crows;
    float* dh;              // [M][H+ctx]
    float* dx;              // [M][3]
    int M, H, ctx, recurrent;
};

__global__ void k_egcl_bnode_out(EgclBNodeOutArgs a) {
    const int W = a.H + a.ctx;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int i = (int)(idx / W), k = (int)(idx - (long long)i * W);
    if (i >= a.M) return;
    float v = 0.0f;
    if (k < a.H) {
        v = (a.recurrent ? a.dout[(size_t)i * a.H + k] : 0.0f) + a.dX[(size_t)i * 2 * a.H + k];
        if (a.T2) v += a.T2[(size_t)i * a.H + k];
        if (k >= a.H - a.ctx) {
            const int kk = k - (a.H - a.ctx);
            if (a.Tc) v += a.Tc[(size_t)i * a.ctx + kk];
            if (a.dh_out) v += a.dh_out[(size_t)i * W + a.H + kk] * (a.nmask ? a.nmask[i] : 1.0f);
        }
    }
    a.dh[(size_t)i * W + k] = v;
    if (k < 3) {
        float s = a.dxs[(size_t)i * 4 + k];
        for (int p = a.rptr[i]; p < a.rptr[i + 1]; ++p) s += a.escal[(size_t)a.rrows[p] * 4 + k];
        for (int p = a.cptr[i]; p < a.cptr[i + 1]; ++p) s -= a.escal[(size_t)a.crows[p] * 4 + k];
        a.dx[(size_t)i * 3 + k] = s;
    }
}
