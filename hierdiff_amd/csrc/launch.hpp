// Which instantiation of a templated kernel family a launch runs, and with how much dynamic LDS.  Host code only; part of
// hierdiff_hip.hip's translation unit: included there once, behind hd_handle, fail, HIP_TRY and ProfScope, which it uses.
//
// Every family has ONE selector, a function of a small key that returns a kernel handle (Kern).  It is the only host code that
// names the family's instantiations and the only place that computes their LDS sizes: a new instantiation is added there, and -
// where a launch needs its LDS limit raised - to the keys the family's prepare_* walks through the same selector.  The size
// policy (which family runs a batch of which size) is the plain functions edge_family and node_path.
// (The HD_DEBUG_KERNELS block of hierdiff_hip.hip names its ablated k_edge instantiations itself.)
#pragma once

// One instantiation and the dynamic LDS it is launched with; fn == nullptr: the family has none for the key.
template <typename A>
struct Kern { void (*fn)(A); int lds; };

template <typename A>
static int launch(const Kern<A>& k, dim3 grid, dim3 block, const A& a, hipStream_t s) {
    if (!k.fn) return fail(HD_E_STATE, "launch: the kernel family has no instantiation for this width / arithmetic / form");
    hipLaunchKernelGGL(k.fn, grid, block, k.lds, s, a);
    return HD_OK;
}

// Raise the dynamic-LDS limit of an instantiation for this device (done once, at hd_create / hd_egcl_create: it is not allowed
// while a stream is capturing, and a launch above 64 KB that was left out fails).
template <typename A>
static int prepare(const Kern<A>& k) {
    if (!k.fn) return fail(HD_E_STATE, "prepare: the kernel family has no instantiation for a key of its list");
    if (k.lds) HIP_TRY(hipFuncSetAttribute((const void*)k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, k.lds));
    return HD_OK;
}

// f(std::integral_constant<int, H>) for the width H of a handle (hd_create admits 32, 64, 128, 256)
template <typename F>
static auto for_width(int H, F&& f) {
    switch (H) {
        case 32: return f(std::integral_constant<int, 32>{});
        case 64: return f(std::integral_constant<int, 64>{});
        case 128: return f(std::integral_constant<int, 128>{});
        default: return f(std::integral_constant<int, 256>{});
    }
}

// f(std::true_type / std::false_type) for a boolean template argument
template <typename F>
static auto for_flag(bool b, F&& f) { return b ? f(std::true_type{}) : f(std::false_type{}); }

// ----------------------------------------------------------------------------- edge kernels (k_edge.hpp, k_edge_split.hpp)

constexpr int edge_lds_bytes(int H) {       // dynamic part: W2 double buffer + wave scratch (w_r/w_d/b2/wa are static)
    return (2 * 32 * H + 2 * H + 4 * 136) * 4;
}

enum class EdgeFam { Tile, Split, Mixed };      // k_edge (one tile per wavefront) | k_edge_split | k_edge_mixed

// prec: arithmetic of the launch (0 fp32, 3 fp16x3); form: the HD_EDGE_* flags of a whole-tile launch (the other families have none)
struct EdgeKey { EdgeFam fam; bool coord; int prec, form; };

// the form of a plain whole-tile launch: exact fp32 is the one family that runs the packed-VALU form (HD_EDGE_PACKED, k_edge.hpp:
// same bits), at the widths of edge_packed_width
constexpr int edge_plain_form(int H, int prec) { return prec == 0 && edge_packed_width(H) ? HD_EDGE_PACKED : 0; }

static Kern<EdgeArgs> edge_kern(int width, const EdgeKey& k) {
    using K = Kern<EdgeArgs>;
    return for_width(width, [&](auto W) { return for_flag(k.coord, [&](auto C) -> K {
        constexpr int H = decltype(W)::value;
        constexpr bool COORD = decltype(C)::value;
        const int lds = edge_lds_bytes(H);
        if constexpr (H >= 128) {               // the column-split families and the fp16x3 training forms exist at these widths only
            if (k.fam == EdgeFam::Split) return k.prec == 3 ? K{k_edge_split<H, COORD, 3>, 0} : K{k_edge_split<H, COORD, 0>, 0};
            if (k.fam == EdgeFam::Mixed) {
                const int ldsm = std::max(lds, edge_split_lds_bytes<H>());
                return k.prec == 3 ? K{k_edge_mixed<H, COORD, 3>, ldsm} : K{k_edge_mixed<H, COORD, 0>, ldsm};
            }
            // training forward in fp16x3 arithmetic: the whole-tile kernel on the unscaled parameters (HD_EDGE_UNSCALED), keeping pre2 or not
            if (k.prec == 3 && k.form == (HD_EDGE_SAVE | HD_EDGE_UNSCALED)) return {k_edge<H, COORD, 3, HD_EDGE_SAVE | HD_EDGE_UNSCALED>, lds};
            if (k.prec == 3 && k.form == HD_EDGE_UNSCALED) return {k_edge<H, COORD, 3, HD_EDGE_UNSCALED>, lds};
        }
        if (k.fam != EdgeFam::Tile) return {nullptr, 0};
        // training forward that keeps pre2 for the backward pass (HD_EDGE_SAVE): the whole-tile kernel's accumulator layout is the
        // saved layout (the caller offers the buffer only where this kernel would run anyway: hd_edge_layer_save_rows)
        if (k.prec == 0 && k.form == HD_EDGE_SAVE) return {k_edge<H, COORD, 0, HD_EDGE_SAVE>, lds};
        if (k.prec == 3 && k.form == 0) return {k_edge<H, COORD, 3>, lds};
        // (the scalar fp32 form stays at every width, although edge_plain_form asks for the packed one where that exists: the build's
        // audit and test_no_register_spills_in_production_kernels check the four plain k_edge<256> forms)
        if (k.prec == 0 && k.form == 0) return {k_edge<H, COORD, 0>, lds};
        if constexpr (edge_packed_width(H)) {
            if (k.prec == 0 && k.form == HD_EDGE_PACKED) return {k_edge<H, COORD, 0, HD_EDGE_PACKED>, lds};
        }
        return {nullptr, 0};
    }); });
}

// The keys a launch can ask for at width H: what edge (below) builds from edge_family and edge_plain_form, and the training forms
// hd_edge_layer_forward_s passes.  A key that a launch starts to build is added HERE too - the selector is shared, this list is not.
static int prepare_edge(int H) {
    for (const bool coord : {false, true}) {
        for (const int prec : {0, 3}) {
            HD_TRY(prepare(edge_kern(H, {EdgeFam::Tile, coord, prec, edge_plain_form(H, prec)})));
            if (H >= 128) for (const EdgeFam fam : {EdgeFam::Split, EdgeFam::Mixed}) HD_TRY(prepare(edge_kern(H, {fam, coord, prec, 0})));
        }
        HD_TRY(prepare(edge_kern(H, {EdgeFam::Tile, coord, 0, HD_EDGE_SAVE})));
        if (H >= 128) for (const int form : {HD_EDGE_SAVE | HD_EDGE_UNSCALED, HD_EDGE_UNSCALED}) HD_TRY(prepare(edge_kern(H, {EdgeFam::Tile, coord, 3, form})));
    }
    return HD_OK;
}

// Which kernel family runs a list of n_tiles edge tiles in arithmetic `prec` (edge below and hd_edge_layer_save_rows ask the same
// question): the column-split kernel, the mix of whole and column-split tiles, or k_edge.
static EdgeFam edge_family(const hd_handle* h, int n_tiles, int prec) {
    if (h->H < 128) return EdgeFam::Tile;
    // at most 512 tiles: one tile per workgroup, columns split over its four wavefronts (k_edge_split.hpp; bit-identical
    // to k_edge in both precision modes, a quarter of the serial MFMA chain per wavefront)
    // measured break-even (profiles/history/r02_split_sweep.log): between 490 and 654 tiles in the 16-bit split modes, between 654 and 870
    // in fp32 (the longer MFMA chain has more to gain from the split)
    if (n_tiles > 0 && n_tiles <= (prec == 0 ? h->split_max_tiles + h->split_max_tiles / 3 : h->split_max_tiles)) return EdgeFam::Split;
    // between one whole-tile workgroup per CU and HD_MIX_MAX_TILES: R * n_cu whole-tile workgroups (every CU the same
    // number) + the remaining tiles as column-split workgroups that back-fill (k_edge_mixed; bit-identical per tile)
    // Measured (profiles/r03_mix_sweep*.log, ms per forward, plain -> mixed): fp32 B = 40 1.89 -> 1.45, 64 1.93 -> 1.88,
    // 96 2.66 -> 2.60, 128 3.29 -> 3.17, 160 4.15 -> 3.89, 192 4.79 -> 4.40, 256 5.41 -> 5.51; the 16-bit split modes gain only
    // while few tiles are left over (B = 40: -14 %; B = 64 ... 256: +2 ... +8 %).  A column-split tile costs about 1.5 x a
    // whole one in SIMD time, so the mix pays when it replaces a badly filled last round: at most 2.9 left-over tiles per
    // CU in fp32, 1.0 in fp16x3.
    const int per_round = 4 * h->n_cu;
    const int left = n_tiles - (n_tiles / per_round) * per_round;
    const bool pays = left > 0 && left * 10 <= (prec == 0 ? 29 : 10) * h->n_cu;
    if (n_tiles > per_round && n_tiles < h->mix_max_tiles && (pays || h->mix_rounds >= 0)) return EdgeFam::Mixed;
    return EdgeFam::Tile;
}

// whole-tile workgroups of a mixed launch: full rounds of one per CU; the grid adds one column-split workgroup per remaining tile
static int edge_mixed_whole_wgs(const hd_handle* h, int n_tiles) {
    int R = n_tiles / (4 * h->n_cu);
    if (h->mix_rounds >= 0) R = std::min(R, h->mix_rounds);
    return R * h->n_cu;
}

#ifdef HD_DEBUG_KERNELS
template <int PREC>
static bool launch_edge_ablated(hd_handle* h, const EdgeArgs& a, hipStream_t s);      // hierdiff_hip.hip
#endif

// One edge layer over the topology's tiles.  `prec` is the arithmetic of THIS launch (0 fp32, 3 fp16x3): the handle's, or the
// opt-in fp16x3 forward of the training path (hd_edge_layer_forward_s) on a handle whose other kernels stay exact fp32.  `form`:
// HD_EDGE_SAVE / HD_EDGE_UNSCALED of a training forward, which always runs the whole-tile kernel; 0: the size policy decides.
static int edge(hd_handle* h, bool coord, const EdgeArgs& a, hipStream_t s, int prec, int form = 0) {
    if (a.n_wg == 0) return HD_OK;
    ProfScope ps(h, s, 0);
    EdgeKey key{EdgeFam::Tile, coord, prec, form};
    EdgeArgs m = a;
    dim3 grid(a.n_wg);
    if (form == 0) {
#ifdef HD_DEBUG_KERNELS
        if (h->H == 256 && h->ablate && !coord && (prec == 3 ? launch_edge_ablated<3>(h, a, s) : launch_edge_ablated<0>(h, a, s))) return HD_OK;
#endif
        key.fam = edge_family(h, a.n_tiles, prec);
        if (key.fam == EdgeFam::Split) grid = dim3(a.n_tiles);
        else if (key.fam == EdgeFam::Mixed) {
            m.n_wg = edge_mixed_whole_wgs(h, a.n_tiles);
            grid = dim3(m.n_wg + (a.n_tiles - 4 * m.n_wg));
        } else key.form = edge_plain_form(h->H, prec);
    }
    return launch(edge_kern(h->H, key), grid, dim3(256), m, s);
}

// ----------------------------------------------------------------------------- edge backward (k_edge_bwd.hpp)

// stage 0 (A) | 1 (B); saved: the forward pass kept pre2 and stage A loads it (one kernel for both arithmetics)
static Kern<EdgeBwdArgs> edge_bwd_kern(int width, bool coord, int stage, int prec, bool saved) {
    using K = Kern<EdgeBwdArgs>;
    return for_width(width, [&](auto W) { return for_flag(coord, [&](auto C) -> K {
        constexpr int H = decltype(W)::value;
        constexpr bool COORD = decltype(C)::value;
        if (stage == 0 && saved) return {k_edge_bwd<H, COORD, 0, 0, true>, 4 * 288 * 4};
        if constexpr (H >= 128) {                   // fp16x3 contraction of stage B (16-wide chunks of 16 H floats)
            if (prec == 3 && stage == 1) return {k_edge_bwd<H, COORD, 1, 3>, (2 * 16 * H + 4 * 288) * 4};
        }
        const int lds = (2 * 32 * H + 4 * 288) * 4;         // two weight chunks + per-wave scratch
        return stage == 0 ? K{k_edge_bwd<H, COORD, 0>, lds} : K{k_edge_bwd<H, COORD, 1>, lds};
    }); });
}

static int prepare_edge_bwd(int H) {
    for (const bool coord : {false, true}) {
        for (const bool saved : {false, true}) HD_TRY(prepare(edge_bwd_kern(H, coord, 0, 0, saved)));
        for (const int prec : {0, 3}) if (prec == 0 || H >= 128) HD_TRY(prepare(edge_bwd_kern(H, coord, 1, prec, false)));
    }
    return HD_OK;
}

// ----------------------------------------------------------------------------- fused node update (k_node.hpp)

// wavefronts per 32-row workgroup: one 32-column tile of an H-wide output each, at most 8 (two per SIMD)
constexpr int node_waves(int H) { return H / 32 < 8 ? H / 32 : 8; }

// mode: 0 fp32 (k_node_f32), 3 fp16 two-piece (k_node; fp16x3 mode at widths >= 128, narrower widths run the fp32 node kernels);
// AB only (!upd), or the update with the AB of the nab layers that follow
static Kern<NodeArgs> node_kern(int width, int mode, bool upd, int nab) {
    return for_width(width, [&](auto W) -> Kern<NodeArgs> {
        constexpr int H = decltype(W)::value, NW = node_waves(H);
        if (mode == 0) {
            const int lds = 32 * ((upd ? 2 * H : H) + 4) * 4 + 32 * (H + 4) * 4;
            if (!upd) return {k_node_f32<H, NW, false, 1>, lds};
            if (nab == 1) return {k_node_f32<H, NW, true, 1>, lds};
            return {k_node_f32<H, NW, true, 2>, lds};
        }
        if constexpr (H >= 128) {
            // region 0: the two fp16 pieces of X; region 1: those of T / the fp32 staging tile
            const int lds = 32 * ((upd ? 2 * H : H) + 8) * 2 * 2 + std::max(32 * (H + 8) * 2 * 2, 32 * (H + 4) * 4);
            if (!upd) return {k_node<H, NW, false, 1>, lds};
            if (nab == 1) return {k_node<H, NW, true, 1>, lds};
            return {k_node<H, NW, true, 2>, lds};
        }
        return {nullptr, 0};
    });
}

static int prepare_node(int H) {
    for (const int mode : {0, 3}) {
        if (mode == 3 && H < 128) continue;
        HD_TRY(prepare(node_kern(H, mode, false, 1)));
        for (const int nab : {1, 2}) HD_TRY(prepare(node_kern(H, mode, true, nab)));
    }
    return HD_OK;
}

// Fused node update in the handle's node arithmetic, 32-row workgroups
static int node_update(hd_handle* h, bool upd, int nab, const NodeArgs& a, hipStream_t s) {
    ProfScope ps(h, s, 1);
    const int nrt = (a.M + 31) / 32;
    return launch(node_kern(h->H, h->node_mode, upd, nab), dim3(8 * ((nrt + 7) / 8)), dim3(64 * node_waves(h->H)), a, s);
}

// ----------------------------------------------------------------------------- node update in three launches (k_node_split.hpp)

// fp16x3, few rows: the node update as three launches (phases 1 - 3) of 32 x 32 output tiles, bit-identical to the fused kernel.
// One 32-column tile per workgroup: two (half the workgroups, half the redundant operand loads; same bits) were measured slower
// at every size from 24 to 64 molecules (profiles/r05_node_split_sweep.log: 0.85 / 0.86 / 0.94 / 0.96 of the fused kernel's forward
// time with one tile, 0.90 / 0.91 / 0.95 / 0.97 with two).
// f32 - exact fp32, widths >= 128, below HD_FUSE_MIN_ROWS rows: the same three launches on k_node_f32's arithmetic (k_node_split_f32)
static Kern<NodeSplitArgs> node_split_kern(int width, bool f32, int phase) {
    return for_width(width, [&](auto W) -> Kern<NodeSplitArgs> {
        constexpr int H = decltype(W)::value;
        if constexpr (H >= 128) {
            if (f32 && phase == 1) return {k_node_split_f32<H, 1>, node_split_f32_lds_bytes<H, 1>()};
            if (f32 && phase == 2) return {k_node_split_f32<H, 2>, node_split_f32_lds_bytes<H, 2>()};
            if (f32 && phase == 3) return {k_node_split_f32<H, 3>, node_split_f32_lds_bytes<H, 3>()};
            if (phase == 1) return {k_node_split<H, 1, 1>, node_split_lds_bytes<H, 1, 1>()};
            if (phase == 2) return {k_node_split<H, 2, 1>, node_split_lds_bytes<H, 2, 1>()};
            if (phase == 3) return {k_node_split<H, 3, 1>, node_split_lds_bytes<H, 3, 1>()};
        }
        return {nullptr, 0};
    });
}

static int launch_node_split(int H, bool f32, int phase, const NodeSplitArgs& a, hipStream_t s) {
    const int nrt = (a.M + 31) / 32;
    const int per = phase == 3 ? 2 * H / 32 * a.n_img : H / 32;
    return launch(node_split_kern(H, f32, phase), dim3(8 * ((nrt + 7) / 8) * per), dim3(256), a, s);
}

static int node_split(hd_handle* h, bool f32, int phase, const NodeSplitArgs& a, hipStream_t s) {
    ProfScope ps(h, s, 1);
    return launch_node_split(h->H, f32, phase, a, s);
}

// both arithmetics (hd_egcl_create needs the fp32 one only and prepares the family as a whole)
static int prepare_node_split(int H) {
    for (const bool f32 : {true, false})
        for (int phase = 1; phase <= 3; ++phase) HD_TRY(prepare(node_split_kern(H, f32, phase)));
    return HD_OK;
}

// ----------------------------------------------------------------------------- node GEMMs (k_gemm_r16.hpp, k_node.hpp)

// 16-row workgroups (RT = 1): 32-row workgroups (RT = 2) were measured: slower up to B = 64, equal above (profiles/r03_r16_sweep2.log)
static Kern<R16Args> r16_kern(int epi, bool agg, int K) {
    const int lds = 16 * (K + 4) * 4;
    if (agg) return {k_gemm_r16<EPI_BIAS_SILU, true, 1>, lds};
    if (epi == EPI_BIAS) return {k_gemm_r16<EPI_BIAS, false, 1>, lds};
    if (epi == EPI_BIAS_SILU) return {k_gemm_r16<EPI_BIAS_SILU, false, 1>, lds};
    return {k_gemm_r16<EPI_RESID_MASK, false, 1>, lds};
}

static int gemm_r16(hd_handle* h, int epi, bool agg, const R16Args& g, hipStream_t s) {
    ProfScope ps(h, s, 1);
    const int wpt = g.Nc >= 128 ? 8 : (g.Nc >> 4);
    return launch(r16_kern(epi, agg, g.K), dim3(((g.M + 15) / 16) * (g.Nc / (16 * wpt)) * g.n_img), dim3(512), g, s);
}

// k_gemm in workgroup tiles of WM x WN wavefronts (32 rows x 32 columns each): 4 x 1 at width 32 (ns = 1), else 2 x 2
template <int WM, int WN>
static Kern<GemmArgs> gemm_kern(int epi, bool cat) {
    if (cat && epi == EPI_RANK1_SILU) return {k_gemm<WM, WN, 1, EPI_RANK1_SILU, true>, 0};
    if (epi == EPI_BIAS_MASK) return {k_gemm<WM, WN, 1, EPI_BIAS_MASK, false>, 0};
    if (cat && epi == EPI_BIAS) return {k_gemm<WM, WN, 1, EPI_BIAS, true>, 0};
    if (cat) return {k_gemm<WM, WN, 1, EPI_BIAS_SILU, true>, 0};
    if (epi == EPI_BIAS_SILU) return {k_gemm<WM, WN, 1, EPI_BIAS_SILU, false>, 0};
    if (epi == EPI_BIAS) return {k_gemm<WM, WN, 1, EPI_BIAS, false>, 0};
    if (epi == EPI_EGCL_PRE) return {k_gemm<WM, WN, 1, EPI_EGCL_PRE, false>, 0};
    return {k_gemm<WM, WN, 1, EPI_RESID_MASK, false>, 0};
}

template <int WM, int WN>
static int launch_gemm_w(int epi, bool cat, const GemmArgs& g, hipStream_t s) {
    const int nrt = (g.M + 32 * WM - 1) / (32 * WM), nct = g.Nc / (32 * WN);
    return launch(gemm_kern<WM, WN>(epi, cat), dim3(8 * ((nrt + 7) / 8) * nct), dim3(WM * WN * 64), g, s);
}
static int launch_gemm(int ns, int epi, bool cat, const GemmArgs& g, hipStream_t s) {
    return ns == 1 ? launch_gemm_w<4, 1>(epi, cat, g, s) : launch_gemm_w<2, 2>(epi, cat, g, s);
}

// ----------------------------------------------------------------------------- training GEMMs (k_tgemm.hpp, k_dw2.hpp)

// a_kc / b_kc: the operand's k stride is 1 (transposed on its way into LDS)
static Kern<TGemmArgs> tgemm_small_kern(bool a_kc, bool b_kc) {
    return for_flag(a_kc, [&](auto A) { return for_flag(b_kc, [&](auto B) {
        return Kern<TGemmArgs>{k_tgemm_small<decltype(A)::value, decltype(B)::value>, 0};
    }); });
}

// fast: full tiles, whole K chunks per slab, 16-byte aligned rows - no bounds checks, no branches around the loads
static Kern<TGemmArgs> tgemm_kern(bool a_kc, bool b_kc, bool fast) {
    return for_flag(a_kc, [&](auto A) { return for_flag(b_kc, [&](auto B) { return for_flag(fast, [&](auto F) {
        return Kern<TGemmArgs>{k_tgemm<decltype(A)::value, decltype(B)::value, decltype(F)::value>, 0};
    }); }); });
}

static Kern<Dw2F16Args> dw2_f16_kern(int H) {       // widths 128 and 256 only (hd_dw2_f16 checks)
    if (H == 256) return {k_dw2_f16<256>, dw2_f16_lds_bytes<256>()};
    return {k_dw2_f16<128>, dw2_f16_lds_bytes<128>()};
}

// ----------------------------------------------------------------------------- per handle

// everything a handle of this width can launch with dynamic LDS (hd_create)
static int prepare_kernels(hd_handle* h) {
    HD_TRY(prepare_node(h->H));
    if (h->H >= 128) HD_TRY(prepare_node_split(h->H));
    HD_TRY(prepare_edge_bwd(h->H));
    return prepare_edge(h->H);
}

// How the node side of a forward of M active rows runs; bit-identical, so a sample's bits do not depend on which one its batch
// size selects (test_fp32_node_paths_agree_bitwise).
enum class NodePath { Split, SplitF32, Fused, R16 };      // k_node_split | k_node_split_f32 | k_node / k_node_f32 | k_gemm_r16 chain

static NodePath node_path(const hd_handle* h, int M) {
    // fp16x3, few rows: the fused kernel's chain per 32-row workgroup (20 - 27 us, a weight stream through one CU) is not hidden
    // when only a few workgroups exist; k_node_split spreads every phase's columns over workgroups (bit-identical)
    if (h->node_mode == 3 && M < h->node_split_max_rows) return NodePath::Split;
    // exact fp32, widths >= 128, below HD_FUSE_MIN_ROWS: k_node_split_f32 (bit-identical to k_node_f32) instead of k_gemm_r16
    if (h->node_mode == 0 && M < h->fuse_min_rows && h->H >= 128 && h->f32_split) return NodePath::SplitF32;
    // fp32 mode, few rows: the fused kernel's serial chain per 32-row workgroup (~50 us) is not hidden by other workgroups
    // (60 of them at B = 64), the k_agg + 3 x k_gemm chain spreads the same work over 64 x 64 tiles.  Both paths are
    // bit-identical (same MFMA order per output element, bias added after the contraction).
    if (h->node_mode != 0 || M >= h->fuse_min_rows) return NodePath::Fused;
    return NodePath::R16;
}
