// The edge kernel (k_edge): edge MLP + attention / coordinate head + per-node partial sums for one 32-edge tile per
// wavefront, two wavefronts per SIMD.  Included through kernels.hpp.
#pragma once
#include "common.hpp"

// ----------------------------------------------------------------------------- edge kernel
// One wavefront = one tile of 32 edge rows x H output columns (NCT accumulators of 32x32).
//   P[e][k]   = silu(A_i[k] + B_j[k] + r_e*w_r[k] + d0_e*w_d[k])      (A operand, built in registers)
//   M[e][c]   = silu(sum_k P[e][k] * W2[c][k] + b2[c])                 (fp32 MFMA, W2 streamed via LDS)
//   GCL  : att_e = sigmoid(wa.M[e] + ba);  partial[i] += M[e]*att_e    (egnn_new.py:35-56)
//   COORD: phi_e = w7.M[e]; trans = u_ij * tanh(phi_e) * range         (egnn_new.py:91-104)
// Rows of a tile are entries of one molecule's edge list (sorted by receiving node i) - or the short tails of several
// molecules at 4-row-aligned offsets; a tile may hold several receiving nodes ("segments") and a node's edges may
// span tiles ("parts").  Where a molecule's edges are cut into tiles depends on that molecule alone, and the per-node
// sums below are invariant under 4-row shifts of a piece inside a tile, so a sample's bits do not depend on its
// batch neighbours (hd_topology_create).

// SiLU of the fp32 edge kernel: the 5-instruction silu_fast (round 3; -2 % on the edge kernel against the
// compensated silu_f of round 2, at unchanged distance to the float64 oracle and with every golden vector still inside the
// bar: the exponent argument is off by <= |x| 1.7e-7 where the value is saturated anyway).  -DHD_F32_SILU=silu_f
// builds the round-2 form.
#ifndef HD_F32_SILU
#define HD_F32_SILU silu_fast
#define HD_F32_SILU_IS_FAST 1          // the epilogue runs silu_fast's five operations stage by stage
#endif

struct EdgeArgs {
    const float* AB;        // [M_pad][2H]: cols <H: W1a.h+b1 ; cols >=H: W1b.h
    const float* wrd;       // [2][H]: w_r (current radial column), w_d (initial distance column)
    const float* W2img;     // [H/32 chunks][32*H] packed
    const float* b2;        // [H]
    const float* wa;        // [H]  (att_mlp.0.weight, or coord_mlp.4.weight)
    const int* ei;          // [E_pad] receiving node (compact)
    const int* ej;          // [E_pad] sending node
    const uint8_t* eseg;    // [E_pad] segment index inside the tile, 255 = padding row
    const int* seg_part;    // [n_tiles][32] part id of each segment of the tile (node-major ids, see hd_topology_create)
    const int* tile_nseg;   // [n_tiles]
    const float* xcur;      // [M_pad][4] coordinates at block start
    const float* x0;        // [M_pad][4] coordinates at network input
    float* part;            // GCL: [P][H];  COORD: [P][4]
    float ba;               // att bias
    const float* ba_ptr;    // optional device copy of the att bias (training: the parameter itself); overrides ba
    float norm_constant;
    float coords_range;     // per-block range
    int attention, use_tanh;
    int n_tiles, n_wg;      // n_wg = number of 128-edge workgroup-tiles
    long long* trace;       // ABL & 16: per wave {start, loop start, loop end, end} cycle stamps
    float w2s_inv;          // PREC 3: 1 / (power-of-two scale of the W2 image)
    float wrmax, wdmax;     // PREC 3: max |w_r|, max |w_d| of this layer (bound on the distance terms of the first layer)
    const float* abmax;     // PREC 3: [M_pad][2] max_k |A_i[k]|, max_k |B_i[k]| of the AB rows (k_ab_rowmax)
    const float* dscal;     // HD_EDGE_UNSCALED: device scalars {2^k, 2^-k, max |w_r|, max |w_d|} (k_f16_prep) instead of w2s_inv, wrmax, wdmax
    float* pre2;            // HD_EDGE_SAVE: [4 n_wg tiles][H/32][4][64 lanes][4] second-layer pre-activations, accumulator order
};

// Flag in the ABL template argument that is not an ablation: the training forward keeps the second-layer pre-activations of
// every edge row (W2 P + b2, the accumulators as they leave the K loop) for the backward pass, which then needs no second
// contraction to get them back (k_edge_bwd<., ., 0, ., true>).  Layout = the accumulator's: one 16-byte store per lane and
// (column tile, row quad), 1 KiB per wavefront instruction; 32 H floats per tile like a row-major [32][H] block.
constexpr int HD_EDGE_SAVE = 256;
// Second such flag (PREC 3 only): the fp16x3 kernel on UNSCALED inputs.  The sampler's fp16x3 mode runs the edge model in a domain
// scaled by c = -log2(e) (the factor sits in the packed weights, so exp(-x) is a bare v_exp_f32); the training forward works on the
// parameters themselves - AB rows from a plain GEMM, w_r / w_d / b2 / wa as they are - and pays the multiplication by c in front of
// every exponential instead (one VALU instruction per activation).  The image scalars come from device memory (EdgeArgs.dscal).
constexpr int HD_EDGE_UNSCALED = 512;
constexpr float HD_NEG_LOG2E = -1.4426950408889634f;
// Third such flag (PREC 0 only): the VALU arithmetic of the exact-fp32 kernel on pairs of values with v_pk_add_f32 / v_pk_mul_f32 /
// v_pk_fma_f32 - the first-layer pre-activations and SiLUs of the operand generation, the mul / +1 / mul stages of the epilogue
// SiLU and the gate dot.  The packed instructions are IEEE per element and every value sees the operations of the scalar form in
// the same order, so the bits are the same; beside the fp32 MFMA (which occupies the same datapath either way) a packed
// instruction costs about 1.1 x a scalar one, i.e. 0.55 x per value.  v_exp_f32 / v_rcp_f32 have no packed form.  Only the plain
// k_edge<H, *, 0> launch selects it (edge_plain_form, launch.hpp: H >= 256); k_edge_mixed, k_edge_split, the training forward and fp16x3
// keep the scalar code.  EXPERIMENTS.md section AN.
constexpr int HD_EDGE_PACKED = 2048;
// the widths whose plain fp32 launch runs the packed form (-DHD_EDGE_NO_PACKED: none, the scalar kernel of a measurement build)
constexpr bool edge_packed_width(int H) {
#ifdef HD_EDGE_NO_PACKED
    return false;
#else
    return H >= 256;
#endif
}
HD_DEVINL f32x2 pk_fma(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }
HD_DEVINL f32x2 pk2(float lo, float hi) { return f32x2{lo, hi}; }
HD_DEVINL f32x2 pk_splat(float v) { return f32x2{v, v}; }


// fp16x3: max_k |A_i[k]| and max_k |B_i[k]| of every AB row (the node-level halves of the first edge Linear) - the per-node part of
// the bound that ranges an edge row's activations.  One wavefront per row: 2H floats, two maxima.
struct AbMaxArgs { const float* AB; float* out; int M, H; };
__global__ void __launch_bounds__(256) k_ab_rowmax(AbMaxArgs a) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= a.M) return;
    const float* r = a.AB + (size_t)row * 2 * a.H;
    float ma = 0.f, mb = 0.f;
    for (int k = 4 * lane; k < a.H; k += 256) {
        const f32x4 va = *reinterpret_cast<const f32x4*>(r + k), vb = *reinterpret_cast<const f32x4*>(r + a.H + k);
#pragma unroll
        for (int j = 0; j < 4; ++j) { ma = fmaxf(ma, fabsf(va[j])); mb = fmaxf(mb, fabsf(vb[j])); }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { ma = fmaxf(ma, __shfl_xor(ma, o)); mb = fmaxf(mb, __shfl_xor(mb, o)); }
    if (lane == 0) { a.out[2 * (size_t)row] = ma; a.out[2 * (size_t)row + 1] = mb; }
}

// Two arithmetics (the retired bf16x3 / bf16x6 codes 1 and 2: EXPERIMENTS.md sections Q, R).
// PREC 0: exact fp32 (v_mfma_f32_32x32x2_f32) - the instruction runs on the SIMD's packed-fp32 datapath and nothing overlaps with it
// (DESIGN.md section 4): unscaled domain, fp32 node GEMMs.
// PREC 3: "fp16x3" - both operands split into an fp16 head and tail (a = ah + al), the product formed as ah*bh + al*bh + ah*bl with
// fp32 accumulation on v_mfma_f32_32x32x16_f16 (three matrix instructions at 16x the fp32 rate), scaled domain: 11 + 11 significant
// bits per operand, so what the three kept terms drop is <= 2^-21 of a product - at the rounding of the fp32 accumulation (measured
// with the real instruction, scratch/mb/f16_denorm.hip: 1.9e-7 rel-L2 against fp64).  fp16 has
// 5 exponent bits, so both operands are brought into range by exact powers of two.  The W2 image is stored x 2^k with its
// largest element in [2^14, 2^15) (per matrix, by the packer).  The activations of an EDGE ROW (i, j) are scaled by
// s = 2^(13 - E), E = floor(log2(bound)), with bound = max_k|A_i[k]| + max_k|B_j[k]| + radial max|w_r| + d0 max|w_d| >=
// |pre-activation| >= |SiLU|: every term is known per edge before the contraction starts (the two row maxima are written by the
// node kernel next to the AB rows, k_node.hpp phase 3, or by k_ab_rowmax), so s x activation < 2^14 ALWAYS - the mode has no range
// assumption left, and rows of small activations are scaled up as much as rows of large ones are scaled down.  s rides in the
// SiLU's reciprocal (`1 + e` becomes fma(e, 1/s, 1/s)); a row of the accumulators holds s 2^k x its pre-activation, and the
// epilogue undoes it in the fused multiply-add that also adds the bias.  Tails below the
// normal range are subnormal fp16 numbers, which the matrix core keeps.

// Four LDS fragment reads / a counted wait that releases them (see k_edge).  The reads are inline asm so
// they stay where they are written (hipcc otherwise sinks every LDS read next to its MFMA to save registers,
// exposing the LDS latency once per fragment); the wait lists the registers as read-write, so their
// consumers cannot be scheduled above it and the compiler cannot touch them between read and wait.
template <typename V, unsigned O0, unsigned O1, unsigned O2, unsigned O3>
HD_DEVINL void lds_read4(V (&f)[4], unsigned addr) {
    asm volatile("ds_read_b128 %0, %4 offset:%5\n\t"
                 "ds_read_b128 %1, %4 offset:%6\n\t"
                 "ds_read_b128 %2, %4 offset:%7\n\t"
                 "ds_read_b128 %3, %4 offset:%8"
                 : "=&v"(f[0]), "=&v"(f[1]), "=&v"(f[2]), "=&v"(f[3])
                 : "v"(addr), "i"(O0), "i"(O1), "i"(O2), "i"(O3));
}
template <typename V, unsigned O>
HD_DEVINL void lds_read1(V& f, unsigned addr) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=&v"(f) : "v"(addr), "i"(O));
}
template <int N, typename V>
HD_DEVINL void lds_wait4(V (&f)[4]) {
    asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]) : "i"(N));
}

// x[lane] + x[lane ^ 32] in every lane, on the VALU (gfx950 v_permlane32_swap: upper half of the first operand
// <-> lower half of the second) instead of a ds_bpermute round trip.  The s_nops cover the VALU-write ->
// permlane-read and permlane-write -> VALU-read hazards, which hipcc does not track through inline asm.
HD_DEVINL float xhalf_sum(float x) {
    float lo = x, hi = x;
    asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(lo), "+v"(hi));
    return lo + hi;
}
// four values per statement: one pair of hazard nops for four swaps
HD_DEVINL void xhalf_sum4(float (&x)[4]) {
    float lo[4], hi[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { lo[k] = x[k]; hi[k] = x[k]; }
    asm("s_nop 1\n\t"
        "v_permlane32_swap_b32 %0, %4\n\tv_permlane32_swap_b32 %1, %5\n\t"
        "v_permlane32_swap_b32 %2, %6\n\tv_permlane32_swap_b32 %3, %7\n\t"
        "s_nop 1"
        : "+v"(lo[0]), "+v"(lo[1]), "+v"(lo[2]), "+v"(lo[3]), "+v"(hi[0]), "+v"(hi[1]), "+v"(hi[2]), "+v"(hi[3]));
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = lo[k] + hi[k];
}

// AB row gathers of the edge kernel: two 16-byte loads (A_i quad, B_j quad) as inline asm, released by a
// hand-counted s_waitcnt vmcnt that names their registers.  Compiler-visible loads cannot be used next to the
// W2 stream: hipcc treats global_load_lds as a second vmcnt event type, assumes mixed events complete out of
// order and waits vmcnt(0) - i.e. for the stream it has just started - before the first use of a gathered row.
// Loads (LDS-DMA included) return in issue order, so "at most N outstanding" releases everything older.
HD_DEVINL void vm_load2(f32x4& va, f32x4& vb, const float* pa, const float* pb) {
    asm volatile("global_load_dwordx4 %0, %2, off\n\t"
                 "global_load_dwordx4 %1, %3, off"
                 : "=&v"(va), "=&v"(vb) : "v"(pa), "v"(pb));
}
// same with a compile-time byte offset (13-bit signed immediate): in a fully unrolled chunk loop hipcc otherwise
// materialises every (chunk, quad) address as its own 64-bit register pair up front and spills them
template <int OFF>
HD_DEVINL void vm_load2o(f32x4& va, f32x4& vb, const float* pa, const float* pb) {
    static_assert(OFF >= 0 && OFF < 4096, "immediate offset out of range");
    asm volatile("global_load_dwordx4 %0, %2, off offset:%4\n\t"
                 "global_load_dwordx4 %1, %3, off offset:%4"
                 : "=&v"(va), "=&v"(vb) : "v"(pa), "v"(pb), "i"(OFF));
}
// AB row gathers of the pipelined kernel go global -> LDS (16 B per lane, lane-linear 1 KiB slots) and are read
// back with ds_read_b128: an asm load with a VGPR destination is unsafe at 256 live VGPRs - hipcc spilled the
// still-in-flight destinations to AGPRs right after the load statement (garbage, and different on every run).
// M0 carries the wave-uniform LDS byte address of the slot and is restored (hipcc reserves it).
HD_DEVINL void vm_glds2(const float* ga, const float* gb, unsigned lds_a, unsigned lds_b) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\t"
                 "s_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\t"
                 "s_mov_b32 m0, %4\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, off\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(ga), "v"(gb), "s"(lds_a), "s"(lds_b));
}
// "at most N VMEM operations outstanding", then fetch an (A quad, B quad) slot pair; lds_ready2 releases the pair
template <int N, unsigned OA, unsigned OB>
HD_DEVINL void lds_read2_after_vm(f32x4& qa, f32x4& qb, unsigned addr) {
    asm volatile("s_waitcnt vmcnt(%3)\n\t"
                 "ds_read_b128 %0, %2 offset:%4\n\t"
                 "ds_read_b128 %1, %2 offset:%5"
                 : "=&v"(qa), "=&v"(qb) : "v"(addr), "i"(N), "i"(OA), "i"(OB));
}
HD_DEVINL void lds_ready2(f32x4& qa, f32x4& qb) { asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(qa), "+v"(qb)); }

template <int N>
HD_DEVINL void vm_wait2(f32x4& va, f32x4& vb) {
    asm volatile("s_waitcnt vmcnt(%2)" : "+v"(va), "+v"(vb) : "i"(N));
}

// byte offset (from the lane's base) of a B fragment inside a chunk image
//   fp16x3: unit u = (k-step, column tile), hl = head (0) / tail (1);   fp32: fragment u = (q, column tile)
template <int NCT>
constexpr unsigned frag_off_f16(int u, int hl) { return (unsigned)((((hl * 2 + u / NCT) * NCT + u % NCT) * 64) * 16); }
constexpr unsigned frag_off_f32(int u) { return (unsigned)(u * 64 * 16); }

// ABL: ablation switches for bottleneck hunting (never set in production launches; env HD_ABLATE, H=256 fp16x3 GCL):
//   1 = skip the epilogue, 2 = skip operand generation (SiLU etc.), 4 = no per-chunk barrier / W2 streaming,
//   8 = no AB row gathers, 16 = record per-wave cycle stamps + HW placement (hd_debug_edge_trace, scratch/edge_trace.py),
//   32 = barrier kept, W2 stream dropped; 64 = W2 stream kept, barrier dropped (round 5: which half of "4" costs what);
//   128 = a quarter of the stream pieces
//
// One workgroup = one 128-edge workgroup-tile (4 wavefronts x 32 edges), two workgroups per CU.  Forms that were built and
// measured slower: a persistent one that walks several tiles per workgroup (spilled); the pipelined one-wave-per-SIMD form of
// round 1 for the two-way loop (scratch/experiments/k_edge_pipelined.hpp); its round-2 successor for fp32 with the epilogue of
// tile t riding under the MFMAs of tile t+1 (scratch/experiments/k_edge_f32p.hpp: bit-identical, 15 % slower - nothing overlaps
// with the fp32 MFMA inside a wavefront).
// The body of k_edge as a device function: `bid` / `nwt` = this workgroup's index among / the number of the launch's
// whole-tile workgroups (k_edge: blockIdx.x / n_wg; k_edge_mixed: the first n_wg blocks of the grid), `smem` the dynamic LDS
// (W2 double buffer + wave scratch), `wrd_s` the separate 4H-float LDS object described below.
// How far the K loop of edge_tile_body is peeled at its end (the forms of the chunk body: see `chunk` there).  2: the last two
// chunks have bodies of their own; 1: only the last chunk has, the second-to-last runs the loop's full body (and fetches 8 rows
// nobody reads); 0: every chunk runs the full body, as before the peel.  The level of an instantiation is the highest at which
// hipcc compiles it without a register spill - a spill next to the hand-counted loads is not an option (hierdiff_amd/build.py:
// audit).  It is a measured table, not a rule derived from the register count: with more straight-line code behind the loop hipcc
// schedules some fp16x3 forms up to the 256-register limit of two waves per SIMD and then spills, also where the same form needs
// only 212 registers one level lower (the unscaled GCL form at H = 128).  Every (instantiation, level) pair: EXPERIMENTS.md
// section AA; taken with -DHD_EDGE_PEEL_LEVEL=n, which forces one level everywhere (measurement builds only: the audit of the
// product build rejects the spilling kernels that level 2 gives).
constexpr int edge_peel_level(int H, int PREC, int ABL) {
#ifdef HD_EDGE_PEEL_LEVEL
    return HD_EDGE_PEEL_LEVEL;
#else
    if (PREC == 0) return 2;                                  // exact fp32: 237-242 registers at H = 256, no spill at any level
    if (ABL & HD_EDGE_UNSCALED) return H >= 256 ? 0 : 1;      // training forward: H = 256 spills at 1 and 2; H = 128 (GCL, not saving) at 2
    return H >= 256 ? 1 : 2;                                  // sampler's fp16x3: H = 256 (coordinate form) spills at 2
#endif
}

template <int H, bool COORD, int PREC, int ABL>
HD_DEVINL void edge_tile_body(const EdgeArgs& a, float* smem, float* wrd_s, const int bid, const int nwt) {
    static_assert(PREC == 0 || PREC == 3, "exact fp32 or fp16x3");
    constexpr int NCT = H / 32;          // 32-column tiles
    constexpr int KC = 32;               // K chunk width
    constexpr int NCH = H / KC;          // K chunks
    constexpr int CHF = 32 * H;          // floats per W2 chunk image
    static_assert(CHF % 1024 == 0, "a chunk image is streamed in 1 KiB pieces, four waves");
    // (ABL bit 128, measurement only: a quarter of the stream - what keeping the W2 heads resident and sharing the tails between
    // eight wavefronts would leave; results are garbage, the time is what the DMA volume is worth)
    constexpr int GL_PER_WAVE = (ABL & 128) ? CHF / (4 * 256) / 4 : CHF / (4 * 256);   // 1 KiB pieces per wave per chunk
    constexpr int LEVEL = edge_peel_level(H, PREC, ABL);
    static_assert(LEVEL >= 0 && LEVEL <= 2, "peel level");
    constexpr bool HAS_PEN = LEVEL >= 2, HAS_LAST = LEVEL >= 1;
    float* wbuf = smem;                   // [2][CHF]
    // w_r / w_d live in their own LDS object (wrd_s: [w_r | w_d | b2 | wa], staged once per workgroup): hipcc makes every
    // compiler-visible LDS read that may alias the destination of an in-flight global_load_lds wait for vmcnt(0) - with
    // one shared array that stalled each chunk on the W2 stream it had just started.
    float* scratch = smem + 2 * CHF + 2 * H;   // per wave: 32 (phi) + 96 (trans) + 8 (seg bytes)

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hh = lane >> 5, n = lane & 31;
    float* my_scr = scratch + wave * 136;
    uint32_t* seg_s = reinterpret_cast<uint32_t*>(my_scr + 128);

    // XCD-aware placement: block b runs on XCD b % 8 and takes the (b / 8)-th workgroup-tile of that XCD's contiguous
    // share of the edge list (neighbouring tiles = same molecule = same AB rows in that XCD's L2)
    int wt;
    {
        const int xcd = bid & 7, slot = bid >> 3;
        const int q = nwt >> 3, r = nwt & 7;
        const int start = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
        const int len = q + (xcd < r ? 1 : 0);
        if (slot >= len) return;
        wt = start + slot;
    }
    long long ts0 = 0, ts1 = 0, ts2 = 0, ts3 = 0, ts4 = 0, ts5 = 0;
    if constexpr (ABL & 16) ts0 = __builtin_readcyclecounter();

    for (int k = tid; k < 2 * H; k += 256) wrd_s[k] = a.wrd[k];
    for (int k = tid; k < H; k += 256) { wrd_s[2 * H + k] = a.b2[k]; wrd_s[3 * H + k] = a.wa[k]; }
    auto issue_chunk = [&](int c, int buf) {
        // this wave's GL_PER_WAVE consecutive 1 KiB pieces of the chunk image; groups of four share one base
        const float* src = a.W2img + (size_t)c * CHF + wave * (GL_PER_WAVE * 256) + lane * 4;
        float* dst = wbuf + buf * CHF + wave * (GL_PER_WAVE * 256);
        static_for<0, GL_PER_WAVE>([&](auto U) {
            constexpr int u = decltype(U)::value;
            glds16o<(u & 3) * 1024>(src + (u >> 2) * 1024, dst + (u >> 2) * 1024);
        });
    };
    issue_chunk(0, 0);

    // per-row metadata of this wavefront's tile (lanes n and n+32 both describe row n)
    const int tile = wt * 4 + wave;
    const bool tile_ok = tile < a.n_tiles;
    int ni = 0, nj = 0;
    uint32_t segb = 255;
    if (tile_ok) {
        const int e = tile * 32 + n;
        ni = a.ei[e]; nj = a.ej[e]; segb = a.eseg[e];
    }

    int gc = 0;                                            // chunk counter: LDS buffer = gc & 1
    f32x4 xi = *reinterpret_cast<const f32x4*>(a.xcur + (size_t)ni * 4);
    f32x4 xj = *reinterpret_cast<const f32x4*>(a.xcur + (size_t)nj * 4);
    f32x4 yi = *reinterpret_cast<const f32x4*>(a.x0 + (size_t)ni * 4);
    f32x4 yj = *reinterpret_cast<const f32x4*>(a.x0 + (size_t)nj * 4);
    const float dx = xi[0] - xj[0], dy = xi[1] - xj[1], dz = xi[2] - xj[2];
    const float radial = dx * dx + dy * dy + dz * dz;
    // coordinate head: unit direction of the edge (egnn_new.py:96-99), zero for padding rows,
    // parked in the wave-private LDS scratch (the slots the epilogue scales in place), not in registers: the
    // kernel sits at the 256-register limit of two waves per SIMD
    if constexpr (COORD) {
        if (hh == 0) {
            const float inv = ((segb != 255) ? 1.0f : 0.0f) / (sqrtf(radial + 1e-8f) + a.norm_constant);
            float* tr = my_scr + 32;
            tr[n * 3 + 0] = dx * inv; tr[n * 3 + 1] = dy * inv; tr[n * 3 + 2] = dz * inv;
        }
    }
    const float ex = yi[0] - yj[0], ey = yi[1] - yj[1], ez = yi[2] - yj[2];
    const float d0 = ex * ex + ey * ey + ez * ez;
    const uint32_t segb_t = segb;
    // fp16x3: this row's activation scale (see the header comment); 1 / (s 2^k) parked for the epilogue, which needs it by row slot
    float f16_inv = 1.0f;
    if constexpr (PREC == 3) {
        const float nodes = a.abmax[2 * (size_t)ni] + a.abmax[2 * (size_t)nj + 1] + HD_F16_FLOOR;
        const float wrmax = (ABL & HD_EDGE_UNSCALED) ? a.dscal[2] : a.wrmax, wdmax = (ABL & HD_EDGE_UNSCALED) ? a.dscal[3] : a.wdmax;
        const float bound = __builtin_fmaf(radial, wrmax, __builtin_fmaf(d0, wdmax, nodes));
        const uint32_t eb = (__builtin_bit_cast(uint32_t, bound) >> 23) & 0xffu;      // bound in [2^(eb-127), 2^(eb-126))
        f16_inv = __builtin_bit_cast(float, (eb - 13u) << 23);                        // 2^-(13 - E), E = eb - 127: bound x s < 2^14
        if (hh == 0) my_scr[n] = f16_inv * ((ABL & HD_EDGE_UNSCALED) ? a.dscal[1] : a.w2s_inv);
    }
    const int pid_l = tile_ok ? a.seg_part[tile * 32 + n] : 0;   // part id of segment n; requested here, used in the epilogue
    const int nseg = tile_ok ? a.tile_nseg[tile] : 0;
    if (hh == 0) reinterpret_cast<uint8_t*>(seg_s)[n] = (uint8_t)segb_t;

    const float* Arow = a.AB + (size_t)ni * (2 * H) + (KC / 2) * hh;
    const float* Brow = a.AB + (size_t)nj * (2 * H) + H + (KC / 2) * hh;
    f32x4 pa[4], pb[4];
    auto rows_issue = [&](int u, int c) {                  // quad u of chunk c (see vm_load2)
        if constexpr (ABL & 8) { pa[u] = f32x4{radial, d0, radial, d0}; pb[u] = pa[u]; }
        else vm_load2(pa[u], pb[u], Arow + KC * c + 4 * u, Brow + KC * c + 4 * u);
    };
    // fp32, HD_EDGE_PACKED: four values as two even-aligned pairs, stage by stage - silu_fast's operations per value in
    // silu_fast's order (20 instructions a quad instead of 32; radial / d0 / the constants are broadcast operands)
    constexpr bool PACKED = PREC == 0 && (ABL & HD_EDGE_PACKED) != 0;
#ifndef HD_F32_SILU_IS_FAST
    static_assert(!PACKED, "the packed form is silu_fast written out");
#endif
    auto make_quad_pk = [&](const f32x4 av, const f32x4 bv, const f32x4 wr4, const f32x4 wd4, float (&P)[16], const int at) {
        f32x2 pre[2], e[2];
#pragma unroll
        for (int p = 0; p < 2; ++p) pre[p] = pk2(av[2 * p], av[2 * p + 1]) + pk2(bv[2 * p], bv[2 * p + 1]);
#pragma unroll
        for (int p = 0; p < 2; ++p) pre[p] = pk_fma(pk_splat(radial), pk2(wr4[2 * p], wr4[2 * p + 1]), pre[p]);
#pragma unroll
        for (int p = 0; p < 2; ++p) pre[p] = pk_fma(pk_splat(d0), pk2(wd4[2 * p], wd4[2 * p + 1]), pre[p]);
#pragma unroll
        for (int p = 0; p < 2; ++p) e[p] = pre[p] * pk_splat(-1.44269502162933349609375f);
#pragma unroll
        for (int p = 0; p < 2; ++p) e[p] = pk2(__builtin_amdgcn_exp2f(e[p][0]), __builtin_amdgcn_exp2f(e[p][1]));
#pragma unroll
        for (int p = 0; p < 2; ++p) e[p] = pk_splat(1.0f) + e[p];
#pragma unroll
        for (int p = 0; p < 2; ++p) e[p] = pk2(__builtin_amdgcn_rcpf(e[p][0]), __builtin_amdgcn_rcpf(e[p][1]));
#pragma unroll
        for (int p = 0; p < 2; ++p) { pre[p] = pre[p] * e[p]; P[at + 2 * p] = pre[p][0]; P[at + 2 * p + 1] = pre[p][1]; }
    };
    // first-layer activations of this lane's edge row for K chunk c (k = 32c + 16*hh + 0..15)
    auto make_P = [&](int c, float (&P)[16]) {             // fp32 mode
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            f32x4 wr4 = *reinterpret_cast<const f32x4*>(wrd_s + 32 * c + 16 * hh + 4 * u);
            f32x4 wd4 = *reinterpret_cast<const f32x4*>(wrd_s + H + 32 * c + 16 * hh + 4 * u);
            if constexpr (PACKED) { make_quad_pk(pa[u], pb[u], wr4, wd4, P, 4 * u); continue; }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float pre = pa[u][j] + pb[u][j];
                pre = __builtin_fmaf(radial, wr4[j], pre);
                pre = __builtin_fmaf(d0, wd4[j], pre);
                P[4 * u + j] = HD_F32_SILU(pre);
            }
        }
    };
    // four values at a time, stage by stage (pre-activation, exp, +1, rcp, product, fp16 split): written per
    // value hipcc schedules each exp -> add -> rcp -> mul chain back to back, which costs an s_nop after every
    // transcendental (forwarding hazard) and a dependent-issue stall per step
    auto make_quad = [&](f32x4 av, f32x4 bv, f32x4 wr4, f32x4 wd4, uint32_t (&hi)[2], uint32_t (&lo)[2]) {
        float pre[4], e[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) pre[j] = av[j] + bv[j];
#pragma unroll
        for (int j = 0; j < 4; ++j) pre[j] = __builtin_fmaf(radial, wr4[j], pre[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j) pre[j] = __builtin_fmaf(d0, wd4[j], pre[j]);
        if constexpr (ABL & 2) {
            f16_split2(av[0], av[1], hi[0], lo[0]);
            f16_split2(av[2], av[3], hi[1], lo[1]);
            return;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) e[j] = __builtin_amdgcn_exp2f((ABL & HD_EDGE_UNSCALED) ? pre[j] * HD_NEG_LOG2E : pre[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j) e[j] = __builtin_fmaf(e[j], f16_inv, f16_inv);
#pragma unroll
        for (int j = 0; j < 4; ++j) e[j] = __builtin_amdgcn_rcpf(e[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j) pre[j] *= e[j];             // row scale x the activation
        f16_split2(pre[0], pre[1], hi[0], lo[0]);
        f16_split2(pre[2], pre[3], hi[1], lo[1]);
    };
    auto make_P_f16 = [&](int c, u32x4 (&ph)[2], u32x4 (&pl)[2]) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const f32x4 wr4 = *reinterpret_cast<const f32x4*>(wrd_s + 32 * c + 16 * hh + 4 * u);
            const f32x4 wd4 = *reinterpret_cast<const f32x4*>(wrd_s + H + 32 * c + 16 * hh + 4 * u);
            uint32_t hi[2], lo[2];
            make_quad(pa[u], pb[u], wr4, wd4, hi, lo);
            ph[u >> 1][2 * (u & 1)] = hi[0]; ph[u >> 1][2 * (u & 1) + 1] = hi[1];
            pl[u >> 1][2 * (u & 1)] = lo[0]; pl[u >> 1][2 * (u & 1) + 1] = lo[1];
        }
    };

    // Software pipeline: the operands of chunk c+1 are produced (VALU) while the matrix pipe works on
    // chunk c; the AB rows are fetched two chunks ahead.
    float Pc[16];
    u32x4 phc[2], plc[2];                  // fp16x3: head / tail of the 16 operand values, 8 fp16 per k-step
    // Both precision modes fetch the AB rows with the hand-counted inline-asm loads (see vm_load2): a compiler-visible
    // load next to the W2 stream makes hipcc wait vmcnt(0) - i.e. for the stream it has just started - every chunk.
    constexpr int NQ = KC / 8;             // row quads per lane per chunk
#pragma unroll
    for (int u = 0; u < NQ; ++u) rows_issue(u, 0);
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(pa[0]), "+v"(pa[1]), "+v"(pa[2]), "+v"(pa[3]),
                                        "+v"(pb[0]), "+v"(pb[1]), "+v"(pb[2]), "+v"(pb[3]));
    __syncthreads();               // chunk 0 landed in every wave's share (w_r / w_d staged on the first pass)
    if constexpr (PREC == 0) make_P(0, Pc);
    else make_P_f16(0, phc, plc);
    if constexpr (NCH > 1 || !HAS_LAST) {   // (one chunk, peeled as the last: nothing follows it, no rows to fetch ahead)
#pragma unroll
        for (int u = 0; u < NQ; ++u) rows_issue(u, NCH > 1 ? 1 : 0);
    }

    // accumulators start at the second layer's bias (saves the H/32 * 16 bias adds of the epilogue).  fp16x3: the bias joins
    // in the epilogue's un-scaling fma, so the accumulators start at zero - and are not initialised at all: the first chunk
    // is peeled off the loop and the first MFMA on each accumulator takes the inline constant 0 as its C operand (128
    // v_mov per tile less; the same bits as adding to a zeroed register).
    #ifdef HD_NO_PEEL
    constexpr bool PEEL = false;
#else
    constexpr bool PEEL = PREC == 3 && !(ABL & 2) && !(ABL & 1024);
#endif
    f32x16 acc[NCT];
    if constexpr (!PEEL) {
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
            const float b2v = PREC == 3 ? 0.0f : wrd_s[2 * H + 32 * ct + n];
            // (8 v_pk_mov_b32 per column tile instead of these 16 v_mov_b32 measured nothing in the packed form: section AN)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ct][r] = b2v;
        }
    }
    if constexpr (ABL & 16) ts1 = __builtin_readcyclecounter();
    // (Unrolling this loop by two with swapped operand sets, to drop the 16 register copies per chunk, was
    // measured twice: 9-17 spilled registers, 125 vs 109 us and later 110-116 vs 103-106 us; fp32 285 vs 278.)
    //
    // Three forms of the chunk body, chosen at compile time (`Kind`), each one branch-free scheduling region:
    //   CH_MID  (chunks 0 .. NCH-3): MFMAs of chunk c, stream of chunk c+1, operands of chunk c+1, row gathers of chunk c+2;
    //   CH_PEN  (chunk NCH-2):       MFMAs of chunk c, stream of chunk c+1, operands of chunk c+1 - there is no chunk c+2;
    //   CH_LAST (chunk NCH-1):       MFMAs only - no stream, no operands, no gathers, no w_r / w_d reads.
    // The runtime loop covers the CH_MID chunks; CH_PEN and CH_LAST follow it as straight-line code.  A workgroup computes one
    // tile per wavefront and ends (k_edge and the whole-tile part of k_edge_mixed alike), so nothing ever follows the last chunk
    // and no peeled form requests chunk 0 again.  That is peel level 2 (edge_peel_level).  At level 1 there is no CH_PEN: chunk
    // NCH-2 runs CH_MID with the rows of "chunk c+2" clamped to the last chunk (8 gathers nobody reads, as before the peel).  At
    // level 0 every chunk runs CH_MID with all three clamps of the loop as it was: operands and rows of the last chunk again, the
    // stream of chunk 0 again.
    constexpr int CH_MID = 0, CH_PEN = 1, CH_LAST = 2;
    auto chunk = [&](auto First, auto Kind, const int c) {
        constexpr bool FIRST = decltype(First)::value;
        constexpr int KIND = decltype(Kind)::value;
        const int buf = (ABL & 4) ? 0 : (gc & 1);
        if constexpr (!(ABL & 4) && !(ABL & 64)) {
            // chunk c landed in LDS and every wave is done with the other buffer.  VMEM operations younger than chunk c's
            // stream, which the body before this one issued:
            //   CH_MID, CH_PEN (c > 0): that body was a CH_MID - the 8 row gathers of chunk c+1                 -> vmcnt(8)
            //   CH_LAST (c > 0), level 2: that body was the CH_PEN, which issues nothing behind its stream      -> vmcnt(0)
            //   CH_LAST (c > 0), level 1: that body was a CH_MID with cn2 clamped - 8 row gathers nobody reads,
            //                             drained behind the loop                                               -> vmcnt(8)
            //   c == 0:                 the prologue's __syncthreads has done it
            if constexpr (KIND == CH_LAST) {
                if constexpr (NCH > 1 && HAS_PEN) asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
                else if constexpr (NCH > 1) asm volatile("s_waitcnt vmcnt(8)\n\ts_barrier" ::: "memory");
            } else if constexpr (KIND == CH_PEN) {
                if constexpr (NCH > 2) asm volatile("s_waitcnt vmcnt(8)\n\ts_barrier" ::: "memory");
            } else {
                if (c > 0) asm volatile("s_waitcnt vmcnt(8)\n\ts_barrier" ::: "memory");
            }
            static_assert(HAS_LAST || KIND == CH_MID, "without a peeled last chunk every chunk runs the full body");
            // The stream of the next chunk is issued unconditionally further down in the forms that have a next chunk:
            // with the stream inside a branch hipcc has to assume "no stream in flight" at the join and waits vmcnt(0) -
            // i.e. for the stream itself - before the first use of the gathered AB rows, every chunk.
        }
        // Branch-free from here to the end of the body (one scheduling region).
        u32x4 phn[2], pln[2];
        // (the clamps exist at the lower peel levels only, where a CH_MID body runs for a chunk that has no chunk c+1 / c+2)
        const int cn1 = HAS_LAST ? c + 1 : (c + 1 < NCH ? c + 1 : NCH - 1);
        const int cn2 = HAS_PEN ? c + 2 : (c + 2 < NCH ? c + 2 : NCH - 1);
        const int cstream = HAS_LAST ? c + 1 : (c + 1 < NCH ? c + 1 : 0);
        // Row quad q of chunk c+1 must have landed.  Outstanding VMEM at that point, oldest first:
        //   CH_MID: quads q..3 of chunk c+1 (8 - 2q loads), the GL_PER_WAVE stream pieces, quads 0..q-1 of chunk c+2 (2q loads)
        //           = 8 + GL_PER_WAVE, of which all but the oldest two may stay                      -> vmcnt(6 + GL_PER_WAVE)
        //   CH_PEN: quads q..3 of chunk c+1 (8 - 2q loads), the GL_PER_WAVE stream pieces - no gathers of a chunk c+2 behind them
        //           = 8 - 2q + GL_PER_WAVE, of which all but the oldest two may stay                 -> vmcnt(6 - 2q + GL_PER_WAVE)
        auto rows_wait = [&](auto Q) {
            constexpr int q = decltype(Q)::value;
            static_assert(KIND != CH_LAST, "the last chunk waits for no rows");
            vm_wait2<(KIND == CH_MID ? 6 : 6 - 2 * q) + GL_PER_WAVE>(pa[q], pb[q]);
        };
        const float* Arow_n2 = Arow + KC * cn2;        // rows of chunk c+2: one address pair per chunk,
        const float* Brow_n2 = Brow + KC * cn2;        // the quad offset rides in the load's immediate
        const float* wb = wbuf + buf * CHF;
        const unsigned wb_lds = (unsigned)(size_t)(__attribute__((address_space(3))) const void*)wb + lane * 16;
        if constexpr (PREC == 0) {
            // chunk image: [4 q][NCT][64 lanes][4 floats]: fragment (q, ct) holds k = 32c + 16h + 4q + j, j = 0..3,
            // of column 32ct + n.  Units of 4 fragments (one q, half of the column tiles) = 16 MFMAs = 1024 matrix-pipe
            // cycles; the next unit's fragments are fetched (inline-asm ds_read_b128, see lds_read4) while the current
            // unit's MFMAs run, the first unit's reads are covered by the stream issue and the operand generation.
            constexpr int HC = NCT >= 4 ? 4 : NCT;          // column tiles per unit
            constexpr int UPQ = NCT / HC;                   // units per q
            constexpr int NU = 4 * UPQ;
            f32x4 f0[4], f1[4];
            auto read_unit = [&](auto U, f32x4 (&f)[4]) {
                constexpr int u = decltype(U)::value, q = u / UPQ, c0 = (u % UPQ) * HC;
                lds_read4<f32x4, frag_off_f32(q * NCT + c0), frag_off_f32(q * NCT + c0 + (HC > 1 ? 1 : 0)),
                          frag_off_f32(q * NCT + c0 + (HC > 2 ? 2 : 0)), frag_off_f32(q * NCT + c0 + (HC > 3 ? 3 : 0))>(f, wb_lds);
            };
            read_unit(std::integral_constant<int, 0>{}, f0);
            if constexpr (KIND != CH_LAST && !(ABL & 4) && !(ABL & 32)) issue_chunk(cstream, buf ^ 1);
            // Operands of chunk c+1 are produced IN PLACE: once the MFMAs of k-quad q have been issued their four operand
            // registers are dead, so quad q of the next chunk is built there (from rows requested one iteration ago) and
            // the rows of chunk c+2 go into the freed row registers (outstanding VMEM at that point: see rows_wait).
            // A unit is pinned instruction by instruction (sched_barrier(0): nothing crosses).  An asm volatile is ordered
            // against other volatile asms only, the MFMA builtins move freely: left alone hipcc hoists the unit's 16 MFMAs
            // above the reads of the next unit (or, with one fence, sinks them below the next unit's wait), so that the wait
            // sits directly behind its reads and every unit starts with an exposed LDS round trip.  Order of a unit:
            //   wait for this unit's fragments; 4 x (MFMA, one fragment read of the next unit); w_r / w_d reads of the quad
            //   produced behind the unit; 12 MFMAs; the quad's operands and the gathers of chunk c+2.
            // Each read is issued in the shadow of a running MFMA and has the remaining 12 to land.  (Edge launch against the
            // unpinned kernel: all four reads in front of the first MFMA +1.3 % - SLOWER; behind the fourth -0.6 %; one behind
            // each of the first four, with the staged epilogue SiLU, -1.8 %.  Operand generation interleaved into the following
            // unit's MFMAs with sched_group_barrier lost against generating it behind the unit in both read placements.
            // EXPERIMENTS.md section AM.)
            static_for<0, NU>([&](auto Uc) {
                constexpr int u = decltype(Uc)::value, q = u / UPQ, c0 = (u % UPQ) * HC;
                f32x4(&cur)[4] = (u & 1) ? f1 : f0;
                f32x4(&nxt)[4] = (u & 1) ? f0 : f1;
                constexpr bool PRODUCE = KIND != CH_LAST && u % UPQ == UPQ - 1;
                lds_wait4<0>(cur);
                __builtin_amdgcn_sched_barrier(0);
                static_for<0, 4>([&](auto Ct) {
                    constexpr int ct = decltype(Ct)::value;
                    if constexpr (ct < HC) acc[c0 + ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(Pc[4 * q], cur[ct][0], acc[c0 + ct], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                    if constexpr (u + 1 < NU) {          // (narrow tiles read a fragment again, as read_unit does)
                        constexpr int qn = (u + 1) / UPQ, cn0 = ((u + 1) % UPQ) * HC;
                        lds_read1<f32x4, frag_off_f32(qn * NCT + cn0 + (ct < HC ? ct : 0))>(nxt[ct], wb_lds);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                });
                f32x4 wr4, wd4;
                if constexpr (PRODUCE) {
                    wr4 = *reinterpret_cast<const f32x4*>(wrd_s + 32 * cn1 + 16 * hh + 4 * q);
                    wd4 = *reinterpret_cast<const f32x4*>(wrd_s + H + 32 * cn1 + 16 * hh + 4 * q);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 1; j < 4; ++j)
#pragma unroll
                    for (int ct = 0; ct < HC; ++ct)
                        acc[c0 + ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(Pc[4 * q + j], cur[ct][j], acc[c0 + ct], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (PRODUCE) {
                    // (packed form: hipcc splits v_pk_*_f32 that follow an MFMA within its latency back into scalar
                    // instructions, to co-issue them - which beside the fp32 MFMA they do not.  Its scan ends at the first
                    // instruction that names the MFMA's destination: an empty asm on the unit's last accumulator.)
                    if constexpr (PACKED) asm volatile("" :: "v"(acc[c0 + HC - 1]));
                    rows_wait(std::integral_constant<int, q>{});
                    if constexpr (PACKED) make_quad_pk(pa[q], pb[q], wr4, wd4, Pc, 4 * q);
                    else {
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            float pre = pa[q][j] + pb[q][j];
                            pre = __builtin_fmaf(radial, wr4[j], pre);
                            pre = __builtin_fmaf(d0, wd4[j], pre);
                            Pc[4 * q + j] = HD_F32_SILU(pre);
                        }
                    }
                    if constexpr (KIND == CH_MID) {
                        if constexpr (ABL & 8) { pa[q] = f32x4{radial, d0, radial, d0}; pb[q] = pa[q]; }
                        else vm_load2o<16 * q>(pa[q], pb[q], Arow_n2, Brow_n2);
                    }
                }
            });
        } else {
            // chunk image: [hi|lo][2 k-steps][NCT][64 lanes][8 fp16]; lane (h, n), element i of step s is
            // W2[32ct + n][32c + 16h + 8s + i] - the same k order as P[8s + i].  Units u = (k-step, ct) of
            // three MFMAs (head*head, tail*head, head*tail) on one accumulator, two units per group.
            constexpr int NG = NCT;                     // 2*NCT units / 2
            // The next chunk's operand generation (VALU) is cut into NG slices, one per MFMA group, so the
            // matrix pipe and the VALU alternate every ~6 MFMAs inside ONE wavefront instead of relying on
            // the phase of the co-resident wavefront.  w_r / w_d come from LDS a slice pair ahead; the AB
            // rows of chunk c+2 replace those of chunk c+1 as soon as their last value has been consumed.
            const float* wr_n = wrd_s + 32 * cn1 + 16 * hh;
            const float* wd_n = wrd_s + H + 32 * cn1 + 16 * hh;
            f32x4 wrq[2], wdq[2];
            if constexpr (KIND != CH_LAST) {
                wrq[0] = *reinterpret_cast<const f32x4*>(wr_n);
                wdq[0] = *reinterpret_cast<const f32x4*>(wd_n);
            }
            f16x8 f0[4], f1[4];
            lds_read4<f16x8, frag_off_f16<NCT>(0, 0), frag_off_f16<NCT>(0, 1), frag_off_f16<NCT>(1, 0), frag_off_f16<NCT>(1, 1)>(f0, wb_lds);
            // the stream for the next chunk goes out behind the first fragment reads: its eight LDS-DMA issues cover
            // the LDS latency the first MFMA group would otherwise wait out
            if constexpr (KIND != CH_LAST && !(ABL & 4) && !(ABL & 32)) issue_chunk(cstream, buf ^ 1);
            static_for<0, NG>([&](auto Gc) {
                constexpr int g = decltype(Gc)::value;
                f16x8(&cur)[4] = (g & 1) ? f1 : f0;
                f16x8(&nxt)[4] = (g & 1) ? f0 : f1;
                lds_wait4<0>(cur);
                if constexpr (g + 1 < NG) {
                    constexpr int u = 2 * (g + 1);
                    lds_read4<f16x8, frag_off_f16<NCT>(u, 0), frag_off_f16<NCT>(u, 1), frag_off_f16<NCT>(u + 1, 0),
                              frag_off_f16<NCT>(u + 1, 1)>(nxt, wb_lds);
                }
                // The group is fenced at both ends, like the fp32 units above: unfenced, hipcc moved the group's MFMAs across
                // the volatile reads and waits until most reads sat directly in front of their wait (fenced: +0.7 % molecules/s).
                __builtin_amdgcn_sched_barrier(0);
                // The next chunk's 8 operand pairs are produced in the FIRST half of the groups and the AB
                // rows of chunk c+2 are requested as soon as a quad of chunk c+1 has been consumed: the
                // per-chunk barrier implies vmcnt(0), so a gather issued late in the chunk would expose its
                // whole L2 latency there.
                constexpr int NGP = NG >= 2 ? NG / 2 : 1;          // groups that produce operands
                constexpr int PPG = 8 / NGP;                       // pairs per producing group
                if constexpr (KIND != CH_LAST && g < NGP) {
                    static_for<0, PPG / 2>([&](auto V) {
                        constexpr int u = g * (PPG / 2) + decltype(V)::value;   // quad u = values 4u .. 4u+3 (pairs 2u, 2u+1)
                        rows_wait(std::integral_constant<int, u>{});             // (the counts: see rows_wait)
                        if constexpr (u + 1 < 4) {                       // w_r / w_d for the following four values
                            wrq[(u + 1) & 1] = *reinterpret_cast<const f32x4*>(wr_n + 4 * (u + 1));
                            wdq[(u + 1) & 1] = *reinterpret_cast<const f32x4*>(wd_n + 4 * (u + 1));
                        }
                        uint32_t hi[2], lo[2];
                        make_quad(pa[u], pb[u], wrq[u & 1], wdq[u & 1], hi, lo);
                        phn[u >> 1][2 * (u & 1)] = hi[0]; phn[u >> 1][2 * (u & 1) + 1] = hi[1];
                        pln[u >> 1][2 * (u & 1)] = lo[0]; pln[u >> 1][2 * (u & 1) + 1] = lo[1];
                        // rows of chunk c+2 into the freed registers (quad offset as an immediate)
                        if constexpr (KIND == CH_MID) {
                            if constexpr (ABL & 8) { pa[u] = f32x4{radial, d0, radial, d0}; pb[u] = pa[u]; }
                            else vm_load2o<16 * u>(pa[u], pb[u], Arow_n2, Brow_n2);
                        }
                    });
                }
                constexpr int u0 = 2 * g, u1 = 2 * g + 1;
                constexpr int s0 = u0 / NCT, c0 = u0 % NCT, s1 = u1 / NCT, c1 = u1 % NCT;
                const f16x8 A_h0 = __builtin_bit_cast(f16x8, phc[s0]), A_l0 = __builtin_bit_cast(f16x8, plc[s0]);
                const f16x8 A_h1 = __builtin_bit_cast(f16x8, phc[s1]), A_l1 = __builtin_bit_cast(f16x8, plc[s1]);
                if constexpr (ABL & 1024) {
                    // measurement only (round 6): NO matrix instruction - operands and fragments are consumed by an empty asm, so
                    // every vector / LDS / memory instruction of the kernel stays: the time of the VECTOR side alone, which is what a
                    // wave-specialised form (one matrix wavefront + one vector wavefront per SIMD) cannot go below
                    asm volatile("" :: "v"(A_h0), "v"(A_l0), "v"(A_h1), "v"(A_l1), "v"(cur[0]), "v"(cur[1]), "v"(cur[2]), "v"(cur[3]));
                } else {
                if constexpr (FIRST && s0 == 0) acc[c0] = mma_f16(A_h0, cur[0], f32x16{});
                else acc[c0] = mma_f16(A_h0, cur[0], acc[c0]);
                if constexpr (FIRST && s1 == 0) acc[c1] = mma_f16(A_h1, cur[2], f32x16{});
                else acc[c1] = mma_f16(A_h1, cur[2], acc[c1]);
                acc[c0] = mma_f16(A_l0, cur[0], acc[c0]);
                acc[c1] = mma_f16(A_l1, cur[2], acc[c1]);
                acc[c0] = mma_f16(A_h0, cur[1], acc[c0]);
                acc[c1] = mma_f16(A_h1, cur[3], acc[c1]);
                }
                if constexpr (KIND != CH_LAST) {         // (the last chunk has no vector work to interleave)
#pragma unroll
                    for (int k = 0; k < 6; ++k) {        // interleave: 1 MFMA, then up to 4 VALU
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                        __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            });
            if constexpr (KIND != CH_LAST) {
#pragma unroll
                for (int st = 0; st < 2; ++st) { phc[st] = phn[st]; plc[st] = pln[st]; }
            }
        }
    };
    using KMid = std::integral_constant<int, CH_MID>;
    using KPen = std::integral_constant<int, CH_PEN>;
    using KLast = std::integral_constant<int, CH_LAST>;
    if constexpr (!HAS_LAST) {
        if constexpr (PEEL) { chunk(std::true_type{}, KMid{}, 0); ++gc; }
#pragma unroll 1
        for (int c = PEEL ? 1 : 0; c < NCH; ++c, ++gc) chunk(std::false_type{}, KMid{}, c);
    } else if constexpr (NCH == 1) {       // the first chunk is the last
        chunk(std::bool_constant<PEEL>{}, KLast{}, 0);
    } else if constexpr (NCH == 2) {       // the first chunk is the second-to-last
        chunk(std::bool_constant<PEEL>{}, std::conditional_t<HAS_PEN, KPen, KMid>{}, 0); ++gc;
        chunk(std::false_type{}, KLast{}, 1);
    } else {
        if constexpr (PEEL) { chunk(std::true_type{}, KMid{}, 0); ++gc; }
#pragma unroll 1
        for (int c = PEEL ? 1 : 0; c < NCH - (HAS_PEN ? 2 : 1); ++c, ++gc) chunk(std::false_type{}, KMid{}, c);
        if constexpr (HAS_PEN) { chunk(std::false_type{}, KPen{}, NCH - 2); ++gc; }
        chunk(std::false_type{}, KLast{}, NCH - 1);
    }

    // Drain before the row registers are reused.  At peel levels 0 and 1 this wait is NEEDED: the last full body (chunk NCH-1 at
    // level 0, chunk NCH-2 at level 1) has issued 8 row gathers nobody reads (cn2 clamped), and the barrier of the last chunk at
    // level 1 waits vmcnt(8) only, which leaves them in flight.  At level 2 nothing is in flight here (the last chunk's barrier
    // waited vmcnt(0), or the prologue did at NCH == 1) and the wait costs nothing; the ablated forms without that barrier drain
    // their stream here.
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(pa[0]), "+v"(pa[1]), "+v"(pa[2]), "+v"(pa[3]),
                                        "+v"(pb[0]), "+v"(pb[1]), "+v"(pb[2]), "+v"(pb[3]));
    if constexpr (ABL & 16) ts2 = __builtin_readcyclecounter();
    if constexpr (ABL & 1024) {             // the untouched accumulators are opaque to the epilogue (no constant folding of its SiLUs)
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) asm volatile("" : "+v"(acc[ct][r]));
    }
    if constexpr (ABL & HD_EDGE_SAVE) {
        static_assert(PREC == 0 || (ABL & HD_EDGE_UNSCALED), "the saved pre-activations are those of the unscaled modes");
        if constexpr (PREC == 3) {         // the un-scaling fma of the epilogue (row scale x image scale out, bias in), done here for all tiles
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                const float b2v = wrd_s[2 * H + 32 * ct + n];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 rs = *reinterpret_cast<const f32x4*>(my_scr + 8 * q + 4 * hh);
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[ct][4 * q + j] = __builtin_fmaf(acc[ct][4 * q + j], rs[j], b2v);
                }
            }
        }
        // every tile of the padded table is written (a tile past n_tiles recomputes node 0's self edge: finite values the
        // backward kernels multiply by zero)
        float* dst = a.pre2 + (size_t)tile * (32 * H) + lane * 4;
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                *reinterpret_cast<f32x4*>(dst + (ct * 4 + q) * 256) = f32x4{acc[ct][4 * q], acc[ct][4 * q + 1], acc[ct][4 * q + 2], acc[ct][4 * q + 3]};
    }
    if (!tile_ok) return;                  // padding tile of the last workgroup: nothing to store
    // (Priority experiments - s_setprio raised for the VALU-only prologue / epilogue, for the MFMA loop, or both - were
    // all null within +-0.5 % on both precisions: profiles/history/r02_ablate_fp32.log.)
    if constexpr (ABL & 1) {
        float sacc = 0.f;
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) sacc += acc[ct][r];
        if (sacc == 123.456f) a.part[lane] = sacc;
        return;
    }

    // ---- epilogue.  acc[ct][r] = row rho(r) = (r&3) + 8*(r>>2) + 4*hh, column 32*ct + n.
    float dot[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) dot[r] = 0.f;
    f32x4 rsc[4];                          // fp16x3: 1 / (row scale x W2 scale) of the 16 rows this lane holds
    if constexpr (PREC == 3) {
#pragma unroll
        for (int q = 0; q < 4; ++q) rsc[q] = *reinterpret_cast<const f32x4*>(my_scr + 8 * q + 4 * hh);
    }
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
        const float wav = wrd_s[3 * H + 32 * ct + n];
        if constexpr (PREC == 0) {
#ifdef HD_F32_SILU_IS_FAST
            // silu_fast stage by stage over the 16 rows of a column tile, like the fp16x3 branch below and for its reason:
            // the same five operations per value, hence the same bits (-0.2 % on the launch, EXPERIMENTS.md section AM)
            if constexpr (PACKED) {
                // the same stages; mul, +1, mul and the gate dot over the pairs (r, r+1) of the column tile's accumulator, which
                // are adjacent, even-aligned registers: 8 packed instructions a stage instead of 16
                f32x2 x2[8], e2[8];
#pragma unroll
                for (int p = 0; p < 8; ++p) { x2[p] = pk2(acc[ct][2 * p], acc[ct][2 * p + 1]); e2[p] = x2[p] * pk_splat(-1.44269502162933349609375f); }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int p = 0; p < 8; ++p) e2[p] = pk2(__builtin_amdgcn_exp2f(e2[p][0]), __builtin_amdgcn_exp2f(e2[p][1]));
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int p = 0; p < 8; ++p) e2[p] = pk_splat(1.0f) + e2[p];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int p = 0; p < 8; ++p) e2[p] = pk2(__builtin_amdgcn_rcpf(e2[p][0]), __builtin_amdgcn_rcpf(e2[p][1]));
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int p = 0; p < 8; ++p) { x2[p] = x2[p] * e2[p]; acc[ct][2 * p] = x2[p][0]; acc[ct][2 * p + 1] = x2[p][1]; }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int p = 0; p < 8; ++p) {
                    const f32x2 d2 = pk_fma(x2[p], pk_splat(wav), pk2(dot[2 * p], dot[2 * p + 1]));
                    dot[2 * p] = d2[0]; dot[2 * p + 1] = d2[1];
                }
                __builtin_amdgcn_sched_barrier(0);
                continue;
            }
            float e[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) e[r] = acc[ct][r] * -1.44269502162933349609375f;
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int r = 0; r < 16; ++r) e[r] = __builtin_amdgcn_exp2f(e[r]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int r = 0; r < 16; ++r) e[r] = 1.0f + e[r];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int r = 0; r < 16; ++r) e[r] = __builtin_amdgcn_rcpf(e[r]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ct][r] *= e[r];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int r = 0; r < 16; ++r) dot[r] = __builtin_fmaf(acc[ct][r], wav, dot[r]);
            __builtin_amdgcn_sched_barrier(0);
#else
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float mv = HD_F32_SILU(acc[ct][r]);
                acc[ct][r] = mv;
                dot[r] = __builtin_fmaf(mv, wav, dot[r]);
            }
#endif
        } else {
            // stage by stage over the 16 rows of a column tile (exp x16, +1 x16, rcp x16, ...): left alone hipcc
            // runs each value's exp -> add -> rcp -> mul chain back to back through one or two registers and
            // the epilogue sits out the transcendental latency ~500 times.
            float e[16];
            if constexpr (!(ABL & HD_EDGE_SAVE)) {
                const float b2v = wrd_s[2 * H + 32 * ct + n];
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[ct][r] = __builtin_fmaf(acc[ct][r], rsc[r >> 2][r & 3], b2v);
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) e[r] = __builtin_amdgcn_exp2f((ABL & HD_EDGE_UNSCALED) ? acc[ct][r] * HD_NEG_LOG2E : acc[ct][r]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int r = 0; r < 16; ++r) e[r] = 1.0f + e[r];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int r = 0; r < 16; ++r) e[r] = __builtin_amdgcn_rcpf(e[r]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ct][r] *= e[r];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int r = 0; r < 16; ++r) dot[r] = __builtin_fmaf(acc[ct][r], wav, dot[r]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    if constexpr (ABL & 16) ts3 = __builtin_readcyclecounter();
    // Row dots: transpose-reduce over the 32 lanes of a half.  Each exchange halves the number of rows a
    // lane still carries (16 -> 8 -> 4 -> 2 -> 1), the last one is a plain butterfly: 16 shuffles instead
    // of 80, and lanes 2r, 2r+1 end up with the complete dot of row slot r, so the sigmoid / tanh input is
    // evaluated once per lane instead of 16 times.
    float rowdot;
    {
        float v8[8], v4[4], v2[2];
        const bool b4 = n & 16, b3 = n & 8, b2_ = n & 4, b1 = n & 2;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float send = b4 ? dot[k] : dot[k + 8];
            const float keep = b4 ? dot[k + 8] : dot[k];
            v8[k] = keep + __shfl_xor(send, 16);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float send = b3 ? v8[k] : v8[k + 4];
            const float keep = b3 ? v8[k + 4] : v8[k];
            v4[k] = keep + __shfl_xor(send, 8);
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const float send = b2_ ? v4[k] : v4[k + 2];
            const float keep = b2_ ? v4[k + 2] : v4[k];
            v2[k] = keep + __shfl_xor(send, 4);
        }
        {
            const float send = b1 ? v2[0] : v2[1];
            const float keep = b1 ? v2[1] : v2[0];
            rowdot = keep + __shfl_xor(send, 2);
        }
        rowdot += __shfl_xor(rowdot, 1);
    }
    if constexpr (ABL & 16) ts4 = __builtin_readcyclecounter();
    const int my_slot = (n >> 1) & 15;                  // this lane holds the dot of row rho(my_slot)

    if (!COORD) {
        // segment byte of each of this lane's 16 rows: rows 8q+4hh .. +3 share one dword
        uint32_t sw[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) sw[q] = seg_s[2 * q + hh];
        float att_mine = 1.0f;
        if (a.attention) {
            const float ba = a.ba_ptr ? *a.ba_ptr : a.ba;
            if constexpr (PREC == 0) att_mine = sigmoid_f(rowdot + ba);
            else att_mine = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f((ABL & HD_EDGE_UNSCALED) ? (rowdot + ba) * HD_NEG_LOG2E : rowdot + ba));   // scaled domain
        }
        float w[16];
        int sg[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            sg[r] = (sw[r >> 2] >> (8 * (r & 3))) & 255;
            const float att = __shfl(att_mine, (lane & 32) | (2 * r));
            w[r] = (sg[r] != 255) ? att : 0.0f;
        }
        if constexpr (ABL & 16) ts5 = __builtin_readcyclecounter();
        // A NaN row (a molecule whose input carries a NaN; also padding rows, which recompute node 0's self edge) would
        // poison the other segments of its tile through 0 * NaN in the masked sums below.  The reference keeps
        // molecules apart (only the velocity is reset batch-wide, en_dynamics.py:109-111), so a tile that holds a NaN
        // row dot takes a select-based form of the same sums: identical bits for finite rows, NaN stays inside its
        // own segments.
        const bool tile_has_nan = __builtin_amdgcn_ballot_w64(rowdot != rowdot) != 0;
        // The sums of segment s run over the row quads that hold a row of s only.  Quad q = rows 8q .. 8q+7 of the tile = this
        // lane's acc[ct][4q .. 4q+3] (either half), segment bytes = the dwords seg_s[2q], seg_s[2q+1]; whether one of those
        // eight bytes equals s is decided on the scalar unit (the zero-byte test on dword ^ s s s s), so the branch is
        // wave-uniform.  A skipped term is fma(0, finite, sum) with a sum that started at +0 and hence is never -0: it returns
        // sum, so the bits are those of the full loop, in which at N = 30 two of three quad passes added nothing.  Segments
        // need not be contiguous for this.  The order of the remaining terms of a sum is unchanged (r ascending).
        uint32_t sq[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) sq[k] = __builtin_amdgcn_readfirstlane(seg_s[k]);
        const int nseg_u = __builtin_amdgcn_readfirstlane(nseg);
        for (int s = 0; s < nseg_u; ++s) {
            float* dst = a.part + (size_t)__builtin_amdgcn_readlane(pid_l, s) * H + n;
            const uint32_t s4 = (uint32_t)s * 0x01010101u;
            float sums[NCT];
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) sums[ct] = 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t x0 = sq[2 * q] ^ s4, x1 = sq[2 * q + 1] ^ s4;
                if (((((x0 - 0x01010101u) & ~x0) | ((x1 - 0x01010101u) & ~x1)) & 0x80808080u) == 0) continue;
                float ws[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) ws[j] = (sg[4 * q + j] == s) ? w[4 * q + j] : 0.0f;
                if (__builtin_expect(tile_has_nan, 0)) {
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            sums[ct] = (sg[4 * q + j] == s) ? __builtin_fmaf(ws[j], acc[ct][4 * q + j], sums[ct]) : sums[ct];
                } else {
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                        for (int j = 0; j < 4; ++j) sums[ct] = __builtin_fmaf(ws[j], acc[ct][4 * q + j], sums[ct]);
                }
            }
            // add the two halves of the wavefront (lane n + 32 hh holds rows 4hh.. of column n)
            if constexpr (NCT % 4 == 0) {
#pragma unroll
                for (int c4 = 0; c4 < NCT; c4 += 4) {
                    float q4[4] = {sums[c4], sums[c4 + 1], sums[c4 + 2], sums[c4 + 3]};
                    xhalf_sum4(q4);
#pragma unroll
                    for (int k = 0; k < 4; ++k) sums[c4 + k] = q4[k];
                }
            } else {
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) sums[ct] = xhalf_sum(sums[ct]);
            }
            if (hh == 0) {
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) dst[32 * ct] = sums[ct];
            }
        }
    } else {
        // phi of row rho(r) is in every lane of half hh; publish per row, then lane n handles row n
        if ((n & 1) == 0) my_scr[(my_slot & 3) + 8 * (my_slot >> 2) + 4 * hh] = rowdot;
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (hh == 0) {
            float phi = my_scr[n];
            float sc = a.use_tanh ? tanhf(phi) * a.coords_range : phi;
            float* tr = my_scr + 32;
            tr[n * 3 + 0] *= sc;
            tr[n * 3 + 1] *= sc;
            tr[n * 3 + 2] *= sc;
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (lane < nseg) {
            const uint8_t* sb = reinterpret_cast<const uint8_t*>(seg_s);
            const float* tr = my_scr + 32;
            float sx = 0.f, sy = 0.f, sz = 0.f;
            for (int rr = 0; rr < 32; ++rr) {
                if (sb[rr] == lane) { sx += tr[rr * 3]; sy += tr[rr * 3 + 1]; sz += tr[rr * 3 + 2]; }
            }
            f32x4 o = {sx, sy, sz, 0.f};
            *reinterpret_cast<f32x4*>(a.part + (size_t)pid_l * 4) = o;      // lane < nseg <= 32: pid_l is segment `lane`'s id
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    if constexpr (ABL & 16) {
        if (lane == 0) {
            long long* t = a.trace + ((size_t)blockIdx.x * 4 + wave) * 8;
            // HW_ID (reg 4) / XCC_ID (reg 20) ride in the top 16 bits of the first two stamps
            const long long hw = __builtin_amdgcn_s_getreg((16 - 1) << 11 | 4) & 0xffff;
            const long long xcc = __builtin_amdgcn_s_getreg((4 - 1) << 11 | 20) & 0xf;
            t[0] = (ts0 & 0xffffffffffffll) | (hw << 48); t[1] = (ts1 & 0xffffffffffffll) | (xcc << 48);
            const long long m48 = 0xffffffffffffll;
            t[2] = ts2 & m48; t[3] = __builtin_readcyclecounter() & m48; t[4] = ts3 & m48; t[5] = ts4 & m48; t[6] = ts5 & m48; t[7] = nseg;
        }
    }
}

template <int H, bool COORD, int PREC, int ABL = 0>
__global__ __launch_bounds__(256, 2) void k_edge(EdgeArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ __attribute__((aligned(16))) float wrd_s[4 * H];
    edge_tile_body<H, COORD, PREC, ABL>(a, smem, wrd_s, blockIdx.x, a.n_wg);
}
