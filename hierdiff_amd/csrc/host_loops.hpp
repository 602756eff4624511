// Host side of the device loops: single sampling steps, schedule and path tables, the replay scaffold of the captured loops, the path
// loop with its entry points, editing and scoring.  Part of hierdiff_hip.hip's translation unit: included there once, behind the
// forward pass and the training primitives, whose objects and helpers (hd_handle, hd_topology, fail, HIP_TRY, forward_impl) it uses.

// ----------------------------------------------------------------------------- sampling maths

static NoiseSrc make_noise(const float* raw_x, const float* raw_h, int rows, uint64_t seed, uint64_t base,
                           uint32_t draw, int share) {
    NoiseSrc n;
    n.raw_x = raw_x; n.raw_h = raw_h; n.rows = rows; n.seed = seed; n.sample_base = base; n.draw = draw; n.share = share;
    return n;
}

// What an emitted step / transition / term works on.  Plain launches: the caller's tensors, and host values for the position
// (`row`, `ro`), the draw and the first sample id.  The captured body: the library-owned copies, the handle's device words, and 0
// for the host values (loop_io_captured).  Fields a loop does not use stay null; the single-step ABI functions fill in a plain one.
struct LoopIO {
    float* z;
    const float *ctx, *tcur;                   // context; network time: a row of d_tau, or the d_tcur word
    const float *ctx_u, *w;                    // guidance: second context, scales
    const uint8_t* fixed;                      // inpainting: mask, known values
    const float* known;
    const uint8_t* fixed_h;                    // ... with per-channel masks (hd_inpaint_parts): `fixed` is the position mask
    const float* xh;                           // scoring: data, accumulator, e_t table
    double* acc;
    float* err;
    int row;                                   // row of the loop's coefficient table
    size_t ro;                                 // injected noise: molecule rows before this position's
    uint32_t draw;
    uint64_t base;
    const int* step;                           // device words (null: plain launches)
    const uint32_t* draw_w;
    const unsigned long long* base_w;
    hipStream_t s;

    bool captured() const { return step != nullptr; }
    // The draw of noise stream i of this position, streams `stride` draws apart: the host value, or the i-th device word (then the
    // value is 0).  Position and sample base need no such fork: `row` / `base` are 0 next to the words `step` / `base_w`.
    struct Draw { uint32_t value; const uint32_t* word; };
    Draw draw_of(int i, uint32_t stride) const { return captured() ? Draw{0u, draw_w + i} : Draw{stride * (uint32_t)i + draw, nullptr}; }
};

// One posterior step zt -> io.z (the loops step in place) in row form `form` (k_post_step).  `coef`: device rows, read at *io.step
// by a captured loop, else row 0 or - coef_rows == B - the molecule's; null: the host `row` by value.  `ns` carries the host draw and
// sample base, `draw_w` the draw's device word (form 2 draws nothing); forms 2 and 3 read the history x_prev and write x_out.
static int step_launch(hd_handle* h, hd_topology* t, const LoopIO& io, int form, const float* zt, const float* eps, const float* coef,
                       int coef_rows, const float* row, const float* x_prev, float* x_out, const NoiseSrc& ns, const uint32_t* draw_w,
                       int mol, int out_stride, int raw_step0) {
    ProfScope ps(h, io.s, 2);
    StepArgs a;
    a.zt = zt; a.eps = eps; a.coef = coef; a.nm = t->nm_bytes; a.x_prev = x_prev; a.x_out = x_out; a.zs = io.z; a.noise = ns;
    a.draw_ptr = draw_w; a.step_ptr = io.step; a.base_ptr = io.base_w; a.raw_step0 = raw_step0;
    for (int k = 0; k < 6; ++k) a.row[k] = (row && k < step_row_width(form)) ? row[k] : 0.f;
    a.coef_rows = coef_rows; a.B = t->B; a.N = t->N; a.D = h->D; a.F = h->F; a.mol = mol; a.out_stride = out_stride;
    const size_t lds = (size_t)mol * a.D * sizeof(float);
    switch (form) {
    case 0: hipLaunchKernelGGL(k_post_step<0>, dim3(t->B), dim3(256), lds, io.s, a); break;
    case 1: hipLaunchKernelGGL(k_post_step<1>, dim3(t->B), dim3(256), lds, io.s, a); break;
    case 2: hipLaunchKernelGGL(k_post_step<2>, dim3(t->B), dim3(256), lds, io.s, a); break;
    default: hipLaunchKernelGGL(k_post_step<3>, dim3(t->B), dim3(256), lds, io.s, a); break;
    }
    HIP_TRY(hipGetLastError());
    return HD_OK;
}

extern "C" int hd_posterior_step(hd_handle* h, hd_topology* topo, const float* zt, const float* eps, const float* coef,
                                 int coef_rows, const float* raw_x, const float* raw_h, int noise_rows, int mol_shape,
                                 float* zs, void* stream) {
    if (!h || !topo) return fail(HD_E_INVALID, "hd_posterior_step: null handle/topology");
    if (!zt || !eps || !coef || !raw_x || !raw_h || !zs) return fail(HD_E_INVALID, "hd_posterior_step: null tensor");
    if (coef_rows != 1 && coef_rows != topo->B) return fail(HD_E_INVALID, "hd_posterior_step: coef_rows must be 1 or B");
    if (noise_rows != 1 && noise_rows != topo->B) return fail(HD_E_INVALID, "hd_posterior_step: noise_rows must be 1 or B");
    const int mol = (mol_shape < 0 || mol_shape > topo->N) ? topo->N : mol_shape;
    if (zs == zt && mol != topo->N) return fail(HD_E_INVALID, "hd_posterior_step: in-place needs mol_shape == N");
    if ((size_t)mol * h->D * sizeof(float) > 64 * 1024) return fail(HD_E_INVALID, "hd_posterior_step: N * D floats exceed one workgroup's LDS");
    HIP_TRY(hipSetDevice(h->device));
    topo_use(topo, (hipStream_t)stream);
    LoopIO io{};
    io.z = zs; io.s = (hipStream_t)stream;
    return step_launch(h, topo, io, 0, zt, eps, coef, coef_rows, nullptr, nullptr, nullptr, make_noise(raw_x, raw_h, noise_rows, 0, 0, 0, 0),
                       nullptr, mol, mol, 0);
}

extern "C" int hd_multistep_step(hd_handle* h, hd_topology* topo, const float* zt, const float* eps, const float* row5,
                                 const float* x_prev, float* x_out, float* zs, void* stream) {
    if (!h || !topo) return fail(HD_E_INVALID, "hd_multistep_step: null handle/topology");
    if (!zt || !eps || !row5 || !x_out || !zs) return fail(HD_E_INVALID, "hd_multistep_step: null tensor");
    if (row5[2] != 0.f && !x_prev) return fail(HD_E_INVALID, "hd_multistep_step: a row with c2 != 0 needs x_prev");
    if (x_out == zt || x_out == eps || x_out == zs || zs == eps || (x_prev && (zs == x_prev || x_prev == zt || x_prev == eps)))
        return fail(HD_E_INVALID, "hd_multistep_step: only zs == zt and x_out == x_prev may alias");
    if ((size_t)topo->N * h->D * sizeof(float) > 64 * 1024) return fail(HD_E_INVALID, "hd_multistep_step: N * D floats exceed one workgroup's LDS");
    HIP_TRY(hipSetDevice(h->device));
    topo_use(topo, (hipStream_t)stream);
    LoopIO io{};
    io.z = zs; io.s = (hipStream_t)stream;
    return step_launch(h, topo, io, 2, zt, eps, nullptr, 1, row5, x_prev, x_out, make_noise(nullptr, nullptr, 1, 0, 0, 0, 0), nullptr, topo->N,
                       topo->N, 0);
}

extern "C" int hd_multistep_sde_step(hd_handle* h, hd_topology* topo, const float* zt, const float* eps, const float* row6,
                                     const float* x_prev, float* x_out, const float* raw_x, const float* raw_h, int noise_rows,
                                     uint64_t seed, uint64_t sample_id_base, uint32_t draw, int share_rows, int mol_shape, float* zs,
                                     void* stream) {
    if (!h || !topo) return fail(HD_E_INVALID, "hd_multistep_sde_step: null handle/topology");
    if (!zt || !eps || !row6 || !x_out || !zs) return fail(HD_E_INVALID, "hd_multistep_sde_step: null tensor");
    if (row6[3] != 0.f && !x_prev) return fail(HD_E_INVALID, "hd_multistep_sde_step: a row with c2 != 0 needs x_prev");
    if ((raw_x == nullptr) != (raw_h == nullptr)) return fail(HD_E_INVALID, "hd_multistep_sde_step: raw_x and raw_h go together");
    if (noise_rows != 1 && noise_rows != topo->B) return fail(HD_E_INVALID, "hd_multistep_sde_step: noise_rows must be 1 or B");
    if (x_out == zt || x_out == eps || x_out == zs || zs == eps || (x_prev && (zs == x_prev || x_prev == zt || x_prev == eps)))
        return fail(HD_E_INVALID, "hd_multistep_sde_step: only zs == zt and x_out == x_prev may alias");
    const int mol = (mol_shape < 0 || mol_shape > topo->N) ? topo->N : mol_shape;
    if ((size_t)mol * h->D * sizeof(float) > 64 * 1024) return fail(HD_E_INVALID, "hd_multistep_sde_step: N * D floats exceed one workgroup's LDS");
    HIP_TRY(hipSetDevice(h->device));
    topo_use(topo, (hipStream_t)stream);
    LoopIO io{};
    io.z = zs; io.s = (hipStream_t)stream;
    return step_launch(h, topo, io, 3, zt, eps, nullptr, 1, row6, x_prev, x_out,
                       make_noise(raw_x, raw_h, noise_rows, seed, sample_id_base, draw, (noise_rows == 1 || share_rows) ? 1 : 0), nullptr, mol,
                       topo->N, 0);
}

extern "C" int hd_final_decode(hd_handle* h, hd_topology* topo, const float* z0, const float* eps, const float* coef3,
                               const float* raw_x, const float* raw_h, int noise_rows, uint64_t seed,
                               uint64_t sample_id_base, uint32_t draw, int share_rows, float* x, float* hfeat,
                               void* stream) {
    if (!h || !topo) return fail(HD_E_INVALID, "hd_final_decode: null handle/topology");
    if (!z0 || !eps || !coef3 || !x || !hfeat) return fail(HD_E_INVALID, "hd_final_decode: null tensor");
    if ((raw_x == nullptr) != (raw_h == nullptr)) return fail(HD_E_INVALID, "hd_final_decode: raw_x and raw_h go together");
    if (raw_x && noise_rows != 1 && noise_rows != topo->B) return fail(HD_E_INVALID, "hd_final_decode: noise_rows must be 1 or B");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    topo_use(topo, s);
    ProfScope ps(h, s, 2);
    DecodeArgs a;
    a.z0 = z0; a.eps = eps; a.nm = topo->nm_bytes; a.x = x; a.hfeat = hfeat;
    a.noise = make_noise(raw_x, raw_h, noise_rows, seed, sample_id_base, draw, share_rows);
    a.sigma_0 = coef3[0]; a.alpha_0 = coef3[1]; a.sigma_x = coef3[2];
    a.B = topo->B; a.N = topo->N; a.D = h->D; a.F = h->F;
    hipLaunchKernelGGL(k_final_decode, dim3((topo->B + 3) / 4), dim3(256), 0, s, a);
    HIP_TRY(hipGetLastError());
    return HD_OK;
}

extern "C" int hd_noise(hd_handle* h, hd_topology* topo, const float* raw_x, const float* raw_h, int noise_rows,
                        uint64_t seed, uint64_t sample_id_base, uint32_t draw, int share_rows, float* z, void* stream) {
    if (!h || !topo || !z) return fail(HD_E_INVALID, "hd_noise: null argument");
    if ((raw_x == nullptr) != (raw_h == nullptr)) return fail(HD_E_INVALID, "hd_noise: raw_x and raw_h go together");
    if (raw_x && noise_rows != 1 && noise_rows != topo->B) return fail(HD_E_INVALID, "hd_noise: noise_rows must be 1 or B");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    topo_use(topo, s);
    ProfScope ps(h, s, 2);
    NoiseArgs a;
    a.nm = topo->nm_bytes; a.z = z; a.noise = make_noise(raw_x, raw_h, noise_rows, seed, sample_id_base, draw, share_rows);
    a.B = topo->B; a.N = topo->N; a.D = h->D; a.F = h->F;
    hipLaunchKernelGGL(k_noise, dim3((topo->B + 3) / 4), dim3(256), 0, s, a);
    HIP_TRY(hipGetLastError());
    return HD_OK;
}

// The one writer of path tables - the caller's or the handle's every-step ones: K validated transitions t_idx[k] -> s_idx[k],
// their rows in the form's width and, for ancestral paths that inpaint, the inpainting rows.
static int set_path_tables(hd_handle* h, PathTables& pt, int K, const int* t_idx, const int* s_idx, const float* rows, const float* rows_ip,
                           int form, bool up) {
    const size_t row_width = (size_t)step_row_width(form);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());                    // a replay may still read the old tables
    pt.d_coef_ip.release();                             // stays empty when no inpainting rows are given
    pt.sched_gen = 0; pt.K = 0;
    pt.t_h.assign(t_idx, t_idx + K);
    pt.s_h.assign(s_idx, s_idx + K);
    if (form == 2 || form == 3) {
        pt.c2_h.resize((size_t)K);
        for (int k = 0; k < K; ++k) pt.c2_h[(size_t)k] = rows[row_width * k + step_row_c2(form)];
    }
    pt.noisy_h.resize((size_t)K);
    for (int k = 0; k < K; ++k) pt.noisy_h[(size_t)k] = form == 0 || (form != 2 && rows[row_width * k + 2] != 0.f);   // k_post_step's `noisy`
    HD_TRY(dev_upload(pt.d_t, pt.t_h));
    HD_TRY(dev_upload(pt.d_s, pt.s_h));
    HD_TRY(dev_upload(pt.d_coef, std::vector<float>(rows, rows + row_width * K)));
    if (rows_ip) HD_TRY(dev_upload(pt.d_coef_ip, std::vector<float>(rows_ip, rows_ip + (size_t)4 * K)));
    pt.K = K; pt.form = form; pt.up = up;
    pt.sched_gen = h->sched_gen;
    pt.gen++;                             // captured graphs hold the old table addresses
    return HD_OK;
}

// rows [T][4] of the schedule in the order of the every-step tables: position k is step s = T - 1 - k
static std::vector<float> rows_reversed(const float* coef4, int T) {
    std::vector<float> r((size_t)4 * T);
    for (int k = 0; k < T; ++k) std::copy(coef4 + (size_t)4 * (T - 1 - k), coef4 + (size_t)4 * (T - k), r.begin() + (size_t)4 * k);
    return r;
}

extern "C" int hd_set_schedule(hd_handle* h, int T, const float* tau, const float* coef4) {
    if (!h || !tau || !coef4 || T < 1) return fail(HD_E_INVALID, "hd_set_schedule: bad argument");
    h->T = 0;                                  // not set until everything below is in place
    h->sched_gen++;                            // captured graphs hold the old table addresses
    // the every-step tables: the identity path T -> T - 1 -> ... -> 0 with the caller's rows (row s of coef4 is the step to s)
    std::vector<int> t_idx((size_t)T), s_idx((size_t)T);
    for (int k = 0; k < T; ++k) { t_idx[(size_t)k] = T - k; s_idx[(size_t)k] = T - 1 - k; }
    HD_TRY(set_path_tables(h, h->every, T, t_idx.data(), s_idx.data(), rows_reversed(coef4, T).data(), nullptr, 0, false));
    h->tau_h.assign(tau, tau + T + 1);
    HD_TRY(dev_upload(h->d_tau, h->tau_h));    // behind set_path_tables' device synchronisation
    h->T = T;
    return HD_OK;
}

// ----------------------------------------------------------------------------- the replay scaffold of the captured loops
//
// The two device loops - the path loop (hd_sample_path*, and hd_sample_loop / hd_sample_loop_inpaint, which run it on the handle's
// every-step tables) and hd_nll_terms - have the same two halves.  Plain launches: the host walks the steps and passes position,
// draw and sample base by value.  use_graph: ONE transition / term is captured into a hipGraph that reads them from the handle's
// device words, works on library-owned copies of every tensor (the caller's move between calls) and is kept in a slot of the
// topology (a GraphSlot) until something in its key changes.  A loop's own part is its key, its slot, its staging copies, its
// state kernel and the emitter of its body; the order of a replaying call is
//     replay_enter -> (grow / allocate owned buffers) -> replay_slot -> staging copies, state kernel
//                  -> replay_run -> copy back -> replay_leave
// No host synchronisation on the way unless a stale graph or buffer has to go: the caller's stream is ordered against the replay
// stream with events.  Everything a body emits is a kernel node.

static LoopIO loop_io_captured(const hd_handle* h, const uint32_t* draw_w, hipStream_t rs) {
    LoopIO io{};
    io.tcur = h->d_tcur; io.step = h->d_step; io.draw_w = draw_w; io.base_w = h->d_base; io.s = rs;
    return io;
}

// The replay stream (the legacy NULL stream cannot be captured: the handle's own stream stands in, ordered behind it), made to
// wait for the handle's latest replay.  The replay state (d_step, d_draw, d_tcur, d_base, ip.d_draw) belongs to the handle: a replay
// issued on another stream - another topology of this handle, or the same one from another caller stream - must have finished
// before this one touches it.
static int replay_enter(hd_handle* h, hipStream_t s, hipStream_t* rs) {
    *rs = s;
    if (s == nullptr) {
        if (!h->own_stream) HIP_TRY(stream_create(h->own_stream, hipStreamNonBlocking));
        *rs = h->own_stream;
        HIP_TRY(hipEventRecord(h->ev_in, s));
        HIP_TRY(hipStreamWaitEvent(*rs, h->ev_in, 0));
    }
    if (h->ev_last_set) HIP_TRY(hipStreamWaitEvent(*rs, h->ev_last, 0));
    return HD_OK;
}

// host wait before something a captured graph holds is freed: a replay may still be running, on any stream
static int replay_quiesce(hd_handle* h, hipStream_t rs) {
    if (h->ev_last_set) HIP_TRY(hipEventSynchronize(h->ev_last));
    HIP_TRY(hipStreamSynchronize(rs));
    return HD_OK;
}

// The one place a slot is filled: a graph built for another key is dropped, and an empty slot captures what `body` emits on rs (an
// int() callable: kernel launches only, profiling brackets off), instantiates it, stores the key and counts the build.
template <typename Key, typename Body>
static int replay_slot(hd_handle* h, hipStream_t rs, GraphSlot<Key>& slot, const Key& want, Body body) {
    if (slot.exec && slot.key == want) return HD_OK;
    if (slot.exec) { HD_TRY(replay_quiesce(h, rs)); slot.exec.reset(); }
    hipGraph_t graph = nullptr;
    HIP_TRY(hipStreamBeginCapture(rs, hipStreamCaptureModeThreadLocal));
    const int was_prof = h->prof;
    h->prof = 0;
    const int rc = body();
    const hipError_t ce = hipStreamEndCapture(rs, &graph);
    h->prof = was_prof;
    if (rc != HD_OK) { if (graph) hipGraphDestroy(graph); return rc; }
    if (ce != hipSuccess) return fail(HD_E_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(ce));
    hipGraphExec_t gx = nullptr;
    const hipError_t ie = hipGraphInstantiate(&gx, graph, nullptr, nullptr, 0);
    hipGraphDestroy(graph);
    if (ie != hipSuccess) return fail(HD_E_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(ie));
    slot.exec.adopt(gx);
    slot.key = want;
    ++slot.builds;
    return HD_OK;
}

static int replay_run(hipGraphExec_t gx, int n, hipStream_t rs) {
    for (int k = 0; k < n; ++k) {
        const hipError_t le = hipGraphLaunch(gx, rs);
        if (le != hipSuccess) return fail(HD_E_HIP, std::string("hipGraphLaunch: ") + hipGetErrorString(le));
    }
    return HD_OK;
}

// mark the end of this replay for the handle's next one, and hand back to the caller's stream
static int replay_leave(hd_handle* h, hipStream_t s, hipStream_t rs) {
    HIP_TRY(hipEventRecord(h->ev_last, rs));
    h->ev_last_set = true;
    if (rs != s) {
        HIP_TRY(hipEventRecord(h->ev_out, rs));
        HIP_TRY(hipStreamWaitEvent(s, h->ev_out, 0));
    }
    return HD_OK;
}

// ----------------------------------------------------------------------------- fragment-constrained sampling (inpainting)

extern "C" int hd_set_inpaint_schedule(hd_handle* h, int T, const float* coef4) {
    if (!h || !coef4 || T < 1) return fail(HD_E_INVALID, "hd_set_inpaint_schedule: bad argument");
    if (h->T < 1) return fail(HD_E_STATE, "hd_set_inpaint_schedule: schedule not set (hd_set_schedule)");
    if (T != h->T) return fail(HD_E_INVALID, "hd_set_inpaint_schedule: T differs from the schedule's (hd_set_schedule)");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    h->ip.sched_gen = 0;
    HD_TRY(dev_upload(h->every.d_coef_ip, rows_reversed(coef4, T)));
    h->ip.sched_gen = h->sched_gen;
    h->ip.gen++;                               // captured graphs hold the old table address
    return HD_OK;
}

// On io.z at position io.row with draw `d`: put the known rows back (io.fixed / io.known; io.fixed_h: per channel), or - `jump` - go
// back to the departure level
// `coef`: the device rows read at the position; null: the host `row` {alpha_s, sigma_s, alpha_t|s, sigma_t|s} by value.
static int inpaint_launch(hd_handle* h, hd_topology* t, const LoopIO& io, bool jump, LoopIO::Draw d, uint64_t seed, const float* coef,
                          const float* row = nullptr) {
    ProfScope ps(h, io.s, 2);
    InpaintArgs a;
    a.z = io.z; a.nm = t->nm_bytes; a.fixed = jump ? nullptr : io.fixed; a.known = jump ? nullptr : io.known; a.coef = coef;
    a.fixed_h = jump ? nullptr : io.fixed_h;
    for (int i = 0; i < 4; ++i) a.row[i] = row ? row[i] : 0.f;
    a.seed = seed; a.sample_base = io.base;
    a.draw = d.value; a.step = io.row; a.draw_ptr = d.word; a.step_ptr = io.step; a.base_ptr = io.base_w;
    a.B = t->B; a.N = t->N; a.D = h->D;
    const size_t lds = (size_t)t->N * h->D * sizeof(float);
    if (jump) hipLaunchKernelGGL(k_inpaint_jump, dim3(t->B), dim3(256), lds, io.s, a);
    else if (io.fixed_h) hipLaunchKernelGGL(k_inpaint_replace<true>, dim3(t->B), dim3(256), lds, io.s, a);
    else hipLaunchKernelGGL(k_inpaint_replace<false>, dim3(t->B), dim3(256), lds, io.s, a);
    HIP_TRY(hipGetLastError());
    return HD_OK;
}

// The checks every inpainting loop makes on its arguments, in the order the header documents.  hd_sample_path_guided words two
// of them its own way, so those texts come from the caller.
static int inpaint_args_check(const char* who, const hd_handle* h, const hd_topology* topo, const float* raw_x, const float* raw_h,
                              int noise_rows, int mol_shape, int resamplings, const float* context, const char* raw_msg,
                              const char* rows_msg) {
    const std::string w(who);
    if (raw_x || raw_h) return fail(HD_E_INVALID, w + raw_msg);
    if (noise_rows != topo->B) return fail(HD_E_INVALID, w + rows_msg);
    if (mol_shape >= 0 && mol_shape < topo->N) return fail(HD_E_INVALID, w + ": fixed tail rows (mol_shape < N) are not supported");
    if (resamplings < 1) return fail(HD_E_INVALID, w + ": resamplings must be >= 1");
    if (h->cfg.context_node_nf > 0 && !context) return fail(HD_E_INVALID, w + ": context required");
    if (!h->cfg.condition_time) return fail(HD_E_INVALID, w + ": needs a time-conditioned model");
    if (((unsigned long long)h->T + 2ULL) * 3ULL * (unsigned long long)resamplings > 0xffffffffULL)
        return fail(HD_E_INVALID, w + ": (T + 2) * 3 * resamplings exceeds the 32-bit draw index");
    if ((size_t)topo->N * h->D * sizeof(float) > 64 * 1024) return fail(HD_E_INVALID, w + ": N * D floats exceed one workgroup's LDS");
    return HD_OK;
}
static const char* const kIpRawMsg = ": injected noise is not supported (counter-based generator only)";
static const char* const kIpRowsMsg = ": noise_rows must be B";

// ... and on the path, before them
static int inpaint_path_check(const char* who, const hd_handle* h, const char* form_msg) {
    const std::string w(who);
    if (h->path.up) return fail(HD_E_INVALID, w + ": the path ascends (hd_set_path_up): inversion fixes no fragments");
    if (h->path.form != 0) return fail(HD_E_INVALID, w + form_msg);
    if (!h->path.d_coef_ip) return fail(HD_E_STATE, w + ": the path was set without inpainting rows (hd_set_path)");
    return HD_OK;
}

// graph replay: room for the draw words of a step's nd = 3 * resamplings noise streams, and the library-owned mask / known values
static int grow_ipdraw(hd_handle* h, hipStream_t rs, int nd) {
    if ((size_t)nd <= h->ip.d_draw.capacity()) return HD_OK;         // (a call that does not inpaint asks for 0 words)
    HD_TRY(replay_quiesce(h, rs));                           // graphs that hold the old address go stale (ip_gen)
    HD_TRY(h->ip.d_draw.alloc((size_t)nd));
    h->ip.gen++;
    return HD_OK;
}

static int inpaint_buffers(const hd_handle* h, hd_topology* t) {
    const size_t BN = (size_t)t->B * t->N;
    HD_TRY(t->ip_fixed.alloc_once(BN));
    return t->ip_known.alloc_once(BN * h->D);
}

// Round j of R behind its posterior step: put the known rows back at the arrival level and - except in the last round - jump back
// to the departure level.  Noise stream 3 * j + m of `stride` draws (LoopIO::draw_of).
static int inpaint_round(hd_handle* h, hd_topology* t, const LoopIO& io, int j, int R, uint32_t stride, uint64_t seed,
                         const float* coef_ip) {
    for (int m = 1; m <= (j < R - 1 ? 2 : 1); ++m)
        HD_TRY(inpaint_launch(h, t, io, m == 2, io.draw_of(3 * j + m, stride), seed, coef_ip));
    return HD_OK;
}

// ----------------------------------------------------------------------------- few-step sampling: the loop on a path

// What every setter of a descending path checks, in this order; `why` closes the range text of the multistep setters.
static int path_down_check(const char* who, const hd_handle* h, int K, const int* t_idx, const int* s_idx, const float* rows, const char* why) {
    const std::string w(who);
    if (!h || !t_idx || !s_idx || !rows || K < 1) return fail(HD_E_INVALID, w + ": bad argument");
    if (h->T < 1) return fail(HD_E_STATE, w + ": schedule not set (hd_set_schedule)");
    if (K > h->T) return fail(HD_E_INVALID, w + ": more transitions than the schedule has steps");
    for (int k = 0; k < K; ++k) {
        if (t_idx[k] > h->T || s_idx[k] < 0 || s_idx[k] >= t_idx[k]) return fail(HD_E_INVALID, w + ": need 0 <= s_idx[k] < t_idx[k] <= T" + why);
        if (k > 0 && t_idx[k] != s_idx[k - 1]) return fail(HD_E_INVALID, w + ": transition k must start where k - 1 arrived");
    }
    return HD_OK;
}

extern "C" int hd_set_path(hd_handle* h, int K, const int* t_idx, const int* s_idx, const float* coef4, int form,
                           const float* coef4_inpaint) {
    if (form != 0 && form != 1) return fail(HD_E_INVALID, "hd_set_path: form must be 0 (ancestral rows) or 1 (linear rows)");
    if (form == 1 && coef4_inpaint) return fail(HD_E_INVALID, "hd_set_path: inpainting rows go with ancestral rows only (form 0)");
    HD_TRY(path_down_check("hd_set_path", h, K, t_idx, s_idx, coef4, ""));
    return set_path_tables(h, h->path, K, t_idx, s_idx, coef4, coef4_inpaint, form, false);
}

// An ascending path into the same tables: transition k leaves from_idx[k] (path_t: network time, as for descending paths) and
// arrives at to_idx[k] (path_s).  Linear rows with c == 0, so k_post_step<1> never looks at the draw word T - to_idx[k].
extern "C" int hd_set_path_up(hd_handle* h, int K, const int* from_idx, const int* to_idx, const float* coef4) {
    if (!from_idx || !to_idx || !coef4 || K < 1) return fail(HD_E_INVALID, "hd_set_path_up: bad argument");
    for (int k = 0; k < K; ++k) {
        if (coef4[(size_t)4 * k + 2] != 0.f || coef4[(size_t)4 * k + 3] != 0.f)
            return fail(HD_E_INVALID, "hd_set_path_up: rows must be {a, b, 0, 0} (the inversion draws nothing)");
        if (from_idx[k] < 0 || from_idx[k] >= to_idx[k]) return fail(HD_E_INVALID, "hd_set_path_up: need 0 <= from_idx[k] < to_idx[k] <= T");
        if (k > 0 && from_idx[k] != to_idx[k - 1]) return fail(HD_E_INVALID, "hd_set_path_up: transition k must start where k - 1 arrived");
    }
    if (!h) return fail(HD_E_INVALID, "hd_set_path_up: null handle");
    if (h->T < 1) return fail(HD_E_STATE, "hd_set_path_up: schedule not set (hd_set_schedule)");
    if (K > h->T) return fail(HD_E_INVALID, "hd_set_path_up: more transitions than the schedule has steps");
    if (to_idx[K - 1] > h->T) return fail(HD_E_INVALID, "hd_set_path_up: need 0 <= from_idx[k] < to_idx[k] <= T");
    return set_path_tables(h, h->path, K, from_idx, to_idx, coef4, nullptr, 1, true);
}

// Descending paths with multistep rows into the same tables: {a, b, c2, p, q} (form 2), and the stochastic {a, b, c, c2, p, q} (form 3).
static int set_path_multistep(const char* who, hd_handle* h, int K, const int* t_idx, const int* s_idx, const float* rows, int form) {
    HD_TRY(path_down_check(who, h, K, t_idx, s_idx, rows, " (a multistep path descends)"));
    if (rows[step_row_c2(form)] != 0.f) return fail(HD_E_INVALID, std::string(who) + ": c2 of row 0 must be 0 (the first transition has no history)");
    return set_path_tables(h, h->path, K, t_idx, s_idx, rows, nullptr, form, false);
}

extern "C" int hd_set_path_multistep(hd_handle* h, int K, const int* t_idx, const int* s_idx, const float* rows5) {
    return set_path_multistep("hd_set_path_multistep", h, K, t_idx, s_idx, rows5, 2);
}

extern "C" int hd_set_path_multistep_sde(hd_handle* h, int K, const int* t_idx, const int* s_idx, const float* rows6) {
    return set_path_multistep("hd_set_path_multistep_sde", h, K, t_idx, s_idx, rows6, 3);
}

extern "C" long long hd_path_graph_builds(const hd_topology* topo) { return topo ? topo->g_path.builds : -1; }

// ----------------------------------------------------------------------------- recording the trajectory of a path loop

extern "C" int hd_set_chain(hd_handle* h, int K, const int* frame_of, const float* alpha_sigma, int frames) {
    if (!h || !frame_of || K < 1 || frames < 1) return fail(HD_E_INVALID, "hd_set_chain: bad argument");
    if (h->path.K < 1 || h->path.sched_gen != h->sched_gen) return fail(HD_E_STATE, "hd_set_chain: path not set for the current schedule (hd_set_path)");
    if (K != h->path.K) return fail(HD_E_INVALID, "hd_set_chain: K differs from the path's (hd_set_path)");
    for (int k = 0; k < K; ++k)
        if (frame_of[k] < -1 || frame_of[k] >= frames) return fail(HD_E_INVALID, "hd_set_chain: need -1 <= frame_of[k] < frames");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());                    // a replay may still read the old tables
    h->chain.d_as.release();                            // stays empty when no {alpha_t, sigma_t} are given
    h->chain.path_gen = 0;
    HD_TRY(dev_upload(h->chain.d_frame, std::vector<int>(frame_of, frame_of + K)));
    if (alpha_sigma) HD_TRY(dev_upload(h->chain.d_as, std::vector<float>(alpha_sigma, alpha_sigma + (size_t)2 * K)));
    h->chain.frames = frames;
    h->chain.path_gen = h->path.gen;
    h->chain.gen++;                            // captured graphs hold the old table addresses
    return HD_OK;
}

extern "C" int hd_chain_attach(hd_topology* topo, float* chain, int frames, int what, float nv0, float nv1, float nb1) {
    if (!topo || !chain || frames < 1) return fail(HD_E_INVALID, "hd_chain_attach: null topology / sink, or frames < 1");
    if (what != 0 && what != 1) return fail(HD_E_INVALID, "hd_chain_attach: what must be 0 (the state) or 1 (the data prediction)");
    topo->chain = ChainSink{chain, frames, what, nv0, nv1, nb1};
    return HD_OK;
}

extern "C" int hd_chain_detach(hd_topology* topo) { if (topo) topo->chain.dst = nullptr; return HD_OK; }

extern "C" long long hd_chain_graph_builds(const hd_topology* topo) { return topo ? topo->g_chain.builds : -1; }

// ----------------------------------------------------------------------------- restraints on the data prediction of a path loop

static bool restraint_row_ok(const float* r) { return r[0] > 0.f && r[1] >= 0.f && r[2] - r[2] == 0.f && r[3] > 0.f; }
static bool steer_row_ok(const float* r) { return r[0] > 0.f && r[1] >= 0.f && r[2] >= 0.f && r[2] - r[2] == 0.f; }

// What the setters of per-transition rows (hd_set_restraint, hd_set_steer) check, in this order; `need` is what a row must satisfy.
static int row_table_check(const char* who, const hd_handle* h, int K, const float* rows, int width, bool (*row_ok)(const float*),
                           const char* need) {
    const std::string w(who);
    if (!h || !rows || K < 1) return fail(HD_E_INVALID, w + ": bad argument");
    if (h->path.K < 1 || h->path.sched_gen != h->sched_gen) return fail(HD_E_STATE, w + ": path not set for the current schedule (hd_set_path)");
    if (K != h->path.K) return fail(HD_E_INVALID, w + ": K differs from the path's (hd_set_path)");
    for (int k = 0; k < K; ++k)
        if (!row_ok(rows + (size_t)width * k)) return fail(HD_E_INVALID, w + need);
    return HD_OK;
}

// K checked rows of `width` floats into a table of the handle, tied to the current path.
static int set_row_table(hd_handle* h, RowTable& tb, int K, const float* rows, int width) {
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());                    // a replay may still read the old rows
    if (!tb.d || tb.K != K) {                           // same K: the table stays where captured transitions expect it
        tb.path_gen = 0; tb.K = 0;
        HD_TRY(tb.d.alloc((size_t)width * K));
        tb.K = K;
        tb.gen++;
    }
    HIP_TRY(hipMemcpy(tb.d, rows, (size_t)width * K * sizeof(float), hipMemcpyHostToDevice));
    tb.path_gen = h->path.gen;
    return HD_OK;
}

extern "C" int hd_set_restraint(hd_handle* h, int K, const float* rows4) {
    HD_TRY(row_table_check("hd_set_restraint", h, K, rows4, 4, restraint_row_ok,
                           ": need alpha_t > 0, sigma_t >= 0, a finite lambda_k and clip_k > 0 (inf: no clip)"));
    return set_row_table(h, h->rs_rows, K, rows4, 4);
}

// A refusal of the entry point `who`; its text is built here, so a call that passes allocates nothing.
static int refuse(int code, const char* who, const std::string& msg) { return fail(code, who + msg); }

// grown when `count` exceeds the capacity (then *moved is set), filled from `src` (device or host memory)
template <typename T>
int DevTable<T>::fill(const T* src, size_t count, bool* moved, hipStream_t s) {
    if (count > this->capacity() || !*this) {
        HIP_TRY(hipDeviceSynchronize());                // a replay may still read the old table
        HD_TRY(this->grow(count, moved));
    }
    if (count) HIP_TRY(hipMemcpyAsync(*this, src, count * sizeof(T), hipMemcpyDefault, s));
    return HD_OK;
}

// The tail of a setter.  `sizes`: {what the last call baked into captured launches, what this call brings}, stored; the generation
// moves when one of them differs or a buffer has `moved`.
static void restraint_bake(std::initializer_list<std::pair<int*, int>> sizes, bool moved, unsigned long long* gen) {
    for (const auto& sz : sizes) {
        moved = moved || *sz.first != sz.second;
        *sz.first = sz.second;
    }
    if (moved) ++*gen;
}

extern "C" int hd_restraint_attach(hd_topology* topo, const float* obs, int obs_rows, int P, const int* pair_idx, const float* pair_f,
                                   int pair_rows, int Q, const int* anc_idx, const float* anc_f, int anc_rows, int A,
                                   const float* scale, int scale_rows, float nv0, void* stream) {
    if (!topo) return fail(HD_E_INVALID, "hd_restraint_attach: null topology");
    if (P < 0 || Q < 0 || A < 0) return fail(HD_E_INVALID, "hd_restraint_attach: P, Q, A must be >= 0");
    if ((P > 0 && !obs) || (Q > 0 && (!pair_idx || !pair_f)) || (A > 0 && (!anc_idx || !anc_f)) || !scale)
        return fail(HD_E_INVALID, "hd_restraint_attach: null table / scale");
    const int B = topo->B;
    for (int r : {obs_rows, pair_rows, anc_rows, scale_rows})
        if (r != 1 && r != B) return fail(HD_E_INVALID, "hd_restraint_attach: every table has 1 row (shared) or B rows");
    if (!(nv0 > 0.f) || !(nv0 - nv0 == 0.f)) return fail(HD_E_INVALID, "hd_restraint_attach: nv0 must be positive and finite");
    if ((size_t)topo->N * 3 * sizeof(float) > 64 * 1024) return fail(HD_E_INVALID, "hd_restraint_attach: N * 3 floats exceed one workgroup's LDS");
    HIP_TRY(hipSetDevice(topo->device));
    hipStream_t s = (hipStream_t)stream;
    topo_use(topo, s);
    RestraintState& r = topo->rs;
    r.on = false;
    bool moved = false;
    HD_TRY(r.obs.fill(obs, (size_t)obs_rows * P * 5, &moved, s));
    HD_TRY(r.pair_idx.fill(pair_idx, (size_t)pair_rows * Q * 2, &moved, s));
    HD_TRY(r.pair_f.fill(pair_f, (size_t)pair_rows * Q * 3, &moved, s));
    HD_TRY(r.anc_idx.fill(anc_idx, (size_t)anc_rows * A, &moved, s));
    HD_TRY(r.anc_f.fill(anc_f, (size_t)anc_rows * A * 5, &moved, s));
    HD_TRY(r.scale.fill(scale, (size_t)scale_rows, &moved, s));
    if (!r.step) { HD_TRY(r.step.alloc((size_t)B * topo->N * 3)); moved = true; }
    restraint_bake({{&r.obs_rows, obs_rows}, {&r.P, P}, {&r.pair_rows, pair_rows}, {&r.Q, Q}, {&r.anc_rows, anc_rows}, {&r.A, A},
                    {&r.scale_rows, scale_rows}}, moved || nv0 != r.nv0, &r.gen);
    r.nv0 = nv0;
    r.frame = 0;                                        // the model's frame, until hd_restraint_frame says otherwise
    r.NF = 0;                                           // no fields, until hd_restraint_fields says otherwise
    r.NT = 0;                                           // no templates, until hd_restraint_templates says otherwise
    r.feat = false;                                     // no features, until hd_restraint_features says otherwise
    r.on = true;
    return HD_OK;
}

extern "C" int hd_restraint_fields(hd_topology* topo, int NF, const float* values, const long long* offsets, const int* dims,
                                   const float* geom, const float* weights, int w_rows, void* stream) {
    if (!topo) return fail(HD_E_INVALID, "hd_restraint_fields: null topology");
    if (NF < 0 || NF > HD_MAX_FIELDS) return fail(HD_E_INVALID, "hd_restraint_fields: NF must be 0 .. 8");
    if (!topo->rs.on) return fail(HD_E_STATE, "hd_restraint_fields: no restraints attached to the topology (hd_restraint_attach)");
    if (NF == 0) { topo->rs.NF = 0; return HD_OK; }
    if (!values || !offsets || !dims || !geom || !weights) return fail(HD_E_INVALID, "hd_restraint_fields: null table");
    if (w_rows != 1 && w_rows != topo->B) return fail(HD_E_INVALID, "hd_restraint_fields: the weights have 1 row (shared) or B rows");
    if (offsets[0] != 0) return fail(HD_E_INVALID, "hd_restraint_fields: offsets[0] must be 0");
    for (int f = 0; f < NF; ++f) {
        long long n = 1;
        for (int c = 0; c < 3; ++c) {
            const int d = dims[f * 3 + c];
            if (d < 2) return fail(HD_E_INVALID, "hd_restraint_fields: every lattice dimension must be >= 2");
            n *= d;
            if (n >= (1LL << 31)) return fail(HD_E_INVALID, "hd_restraint_fields: a lattice holds fewer than 2^31 values");
            const float hc = geom[f * 8 + 3 + c], oc = geom[f * 8 + c];
            if (!(hc > 0.f) || !(hc - hc == 0.f)) return fail(HD_E_INVALID, "hd_restraint_fields: every spacing must be positive and finite");
            if (!(oc - oc == 0.f)) return fail(HD_E_INVALID, "hd_restraint_fields: the origin must be finite");
        }
        for (int c = 6; c < 8; ++c) {
            const float v = geom[f * 8 + c];
            if (!(v >= 0.f) || !(v - v == 0.f)) return fail(HD_E_INVALID, "hd_restraint_fields: k and wall must be >= 0 and finite");
        }
        if (offsets[f + 1] - offsets[f] != n) return fail(HD_E_INVALID, "hd_restraint_fields: offsets[f + 1] - offsets[f] must be n0 n1 n2 of field f");
    }
    HIP_TRY(hipSetDevice(topo->device));
    hipStream_t s = (hipStream_t)stream;
    topo_use(topo, s);
    RestraintState& r = topo->rs;
    r.NF = 0;
    bool moved = false;
    if (!r.fld_geom) {                                  // all three or none: moved in once every allocation succeeded
        DevBuf<long long> off;
        DevBuf<int> fdims;
        DevBuf<float> fgeom;
        HD_TRY(off.alloc((size_t)HD_MAX_FIELDS + 1));
        HD_TRY(fdims.alloc((size_t)HD_MAX_FIELDS * 3));
        HD_TRY(fgeom.alloc((size_t)HD_MAX_FIELDS * 8));
        r.fld_off = std::move(off); r.fld_dims = std::move(fdims); r.fld_geom = std::move(fgeom);
        moved = true;
    }
    HD_TRY(r.fld_v.fill(values, (size_t)offsets[NF], &moved, s));
    HD_TRY(r.fld_w.fill(weights, (size_t)w_rows * NF * topo->N, &moved, s));
    // (host arrays: pageable sources are staged before the call returns)
    HIP_TRY(hipMemcpyAsync(r.fld_off, offsets, ((size_t)NF + 1) * sizeof(long long), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(r.fld_dims, dims, (size_t)NF * 3 * sizeof(int), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(r.fld_geom, geom, (size_t)NF * 8 * sizeof(float), hipMemcpyHostToDevice, s));
    restraint_bake({{&r.fld_NF, NF}, {&r.fld_w_rows, w_rows}}, moved, &r.fld_gen);
    r.NF = NF;
    return HD_OK;
}

extern "C" int hd_restraint_templates(hd_topology* topo, int NT, int rows, int M, const int* idx, const float* f, const float* geom,
                                      void* stream) {
    if (!topo) return fail(HD_E_INVALID, "hd_restraint_templates: null topology");
    if (NT < 0 || NT > HD_MAX_TEMPLATES) return fail(HD_E_INVALID, "hd_restraint_templates: NT must be 0 .. 4");
    if (!topo->rs.on) return fail(HD_E_STATE, "hd_restraint_templates: no restraints attached to the topology (hd_restraint_attach)");
    if (NT == 0) { topo->rs.NT = 0; return HD_OK; }
    if (M < 1) return fail(HD_E_INVALID, "hd_restraint_templates: M must be >= 1");
    if (rows != 1 && rows != topo->B) return fail(HD_E_INVALID, "hd_restraint_templates: the tables have 1 row (shared) or B rows");
    if (!idx || !f || !geom) return fail(HD_E_INVALID, "hd_restraint_templates: null table");
    for (int t = 0; t < NT; ++t) {
        const float k = geom[2 * t], fit = geom[2 * t + 1];
        if (!(k >= 0.f) || !(k - k == 0.f)) return fail(HD_E_INVALID, "hd_restraint_templates: k must be >= 0 and finite");
        if (fit != 0.f && fit != 1.f) return fail(HD_E_INVALID, "hd_restraint_templates: fit is 0 (rigid) or 1 (translation)");
    }
    const size_t cnt = (size_t)rows * NT * M;
    for (size_t e = 0; e < cnt; ++e) {
        const float* r = f + e * 4;
        if (!(r[0] - r[0] == 0.f) || !(r[1] - r[1] == 0.f) || !(r[2] - r[2] == 0.f))
            return fail(HD_E_INVALID, "hd_restraint_templates: the template positions must be finite");
        if (!(r[3] >= 0.f) || !(r[3] - r[3] == 0.f)) return fail(HD_E_INVALID, "hd_restraint_templates: every weight must be >= 0 and finite");
    }
    HIP_TRY(hipSetDevice(topo->device));
    hipStream_t s = (hipStream_t)stream;
    topo_use(topo, s);
    RestraintState& r = topo->rs;
    r.NT = 0;
    bool moved = false;
    if (!r.tpl_geom) { HD_TRY(r.tpl_geom.alloc((size_t)HD_MAX_TEMPLATES * 2)); moved = true; }
    // (host arrays: pageable sources are staged before the call returns)
    HD_TRY(r.tpl_idx.fill(idx, cnt, &moved, s));
    HD_TRY(r.tpl_f.fill(f, cnt * 4, &moved, s));
    HIP_TRY(hipMemcpyAsync(r.tpl_geom, geom, (size_t)NT * 2 * sizeof(float), hipMemcpyHostToDevice, s));
    restraint_bake({{&r.tpl_NT, NT}, {&r.tpl_M, M}, {&r.tpl_rows, rows}}, moved, &r.tpl_gen);
    r.NT = NT;
    return HD_OK;
}

extern "C" int hd_restraint_features(hd_topology* topo, const float* lo, const float* hi, const float* k, int band_rows, int W,
                                     const float* coef, const float* sum_f, int sum_rows, int S, float nv1, float nb1, float ratio,
                                     void* stream) {
    const char* who = "hd_restraint_features";
    if (!topo) return refuse(HD_E_INVALID, who, ": null topology");
    if (W < 0 || W > topo->N) return refuse(HD_E_INVALID, who, ": W must be 0 .. N (nodes i >= W have no band)");
    if (S < 0 || S > HD_MAX_FEATURE_SUMS) return refuse(HD_E_INVALID, who, ": S must be 0 .. 8");
    if (!topo->rs.on) return refuse(HD_E_STATE, who, ": no restraints attached to the topology (hd_restraint_attach)");
    if (W == 0 && S == 0) { topo->rs.feat = false; return HD_OK; }
    const int F = topo->h->D - 3;
    if (F < 1) return refuse(HD_E_INVALID, who, ": the model has no feature columns");
    if ((W > 0 && (!lo || !hi || !k)) || (S > 0 && (!coef || !sum_f))) return refuse(HD_E_INVALID, who, ": null table");
    if ((W > 0 && band_rows != 1 && band_rows != topo->B) || (S > 0 && sum_rows != 1 && sum_rows != topo->B))
        return refuse(HD_E_INVALID, who, ": every table has 1 row (shared) or B rows");
    for (float v : {nv1, nb1, ratio})
        if (!(v - v == 0.f)) return refuse(HD_E_INVALID, who, ": nv1, nb1 and ratio must be finite");
    if (W == 0) band_rows = 1;
    if (S == 0) sum_rows = 1;
    const size_t nb = (size_t)band_rows * W * F, nc = (size_t)sum_rows * S * F, ns = (size_t)sum_rows * S;
    for (size_t e = 0; e < nb; ++e) {
        if (!(k[e] - k[e] == 0.f)) return refuse(HD_E_INVALID, who, ": every k must be finite");
        if (lo[e] != lo[e] || hi[e] != hi[e]) return refuse(HD_E_INVALID, who, ": a bound may be infinite, not NaN");
        if (lo[e] > hi[e]) return refuse(HD_E_INVALID, who, ": lo > hi");
    }
    for (size_t e = 0; e < nc; ++e)
        if (!(coef[e] - coef[e] == 0.f)) return refuse(HD_E_INVALID, who, ": every coefficient must be finite");
    for (size_t e = 0; e < ns; ++e) {
        const float* r = sum_f + 4 * e;
        if (!(r[2] - r[2] == 0.f)) return refuse(HD_E_INVALID, who, ": every k must be finite");
        if (r[0] != r[0] || r[1] != r[1]) return refuse(HD_E_INVALID, who, ": a bound may be infinite, not NaN");
        if (r[0] > r[1]) return refuse(HD_E_INVALID, who, ": lo > hi");
        if (r[3] != 0.f && r[3] != 1.f) return refuse(HD_E_INVALID, who, ": reduce is 0 (sum) or 1 (mean)");
    }
    if ((size_t)topo->N * topo->h->D * sizeof(float) > 64 * 1024) return refuse(HD_E_INVALID, who, ": N * D floats exceed one workgroup's LDS");
    HIP_TRY(hipSetDevice(topo->device));
    hipStream_t s = (hipStream_t)stream;
    topo_use(topo, s);
    RestraintState& r = topo->rs;
    r.feat = false;
    bool moved = false;
    // (host arrays: pageable sources are staged before the call returns)
    HD_TRY(r.ft_lo.fill(lo, nb, &moved, s));
    HD_TRY(r.ft_hi.fill(hi, nb, &moved, s));
    HD_TRY(r.ft_k.fill(k, nb, &moved, s));
    HD_TRY(r.ft_coef.fill(coef, nc, &moved, s));
    HD_TRY(r.ft_sum.fill(sum_f, ns * 4, &moved, s));
    restraint_bake({{&r.ft_band_rows, band_rows}, {&r.ft_W, W}, {&r.ft_sum_rows, sum_rows}, {&r.ft_S, S}},
                   moved || nv1 != r.ft_nv1 || nb1 != r.ft_nb1 || ratio != r.ft_ratio, &r.feat_gen);
    r.ft_nv1 = nv1; r.ft_nb1 = nb1; r.ft_ratio = ratio;
    r.feat = true;
    return HD_OK;
}

extern "C" int hd_restraint_frame(hd_topology* topo, int frame) {
    if (!topo) return fail(HD_E_INVALID, "hd_restraint_frame: null topology");
    if (frame != 0 && frame != 1) return fail(HD_E_INVALID, "hd_restraint_frame: frame is 0 (the model's) or 1 (the known fragments')");
    if (!topo->rs.on) return fail(HD_E_STATE, "hd_restraint_frame: no restraints attached to the topology (hd_restraint_attach)");
    topo->rs.frame = frame;                             // part of the graph key (RestraintKey::frame)
    return HD_OK;
}

extern "C" int hd_restraint_detach(hd_topology* topo) { if (topo) topo->rs.on = false; return HD_OK; }

// The kernels' views of the state (k_restrain.hpp): NF / NT are what is attached now, not what was last baked in.
static RestraintTables restraint_tables(const hd_topology* t) {
    const RestraintState& s = t->rs;
    RestraintTables r;
    r.obs = s.obs; r.pair_idx = s.pair_idx; r.pair_f = s.pair_f; r.anc_idx = s.anc_idx; r.anc_f = s.anc_f;
    r.obs_rows = s.obs_rows; r.P = s.P; r.pair_rows = s.pair_rows; r.Q = s.Q; r.anc_rows = s.anc_rows; r.A = s.A;
    r.fld_v = s.fld_v; r.fld_off = s.fld_off; r.fld_dims = s.fld_dims; r.fld_geom = s.fld_geom; r.fld_w = s.fld_w;
    r.fld_w_rows = s.fld_w_rows; r.NF = s.NF;
    return r;
}

static TemplateTables template_tables(const hd_topology* t) {
    const RestraintState& s = t->rs;
    TemplateTables r;
    r.idx = s.tpl_idx; r.f = s.tpl_f; r.geom = s.tpl_geom;
    r.rows = s.tpl_rows; r.NT = s.NT; r.M = s.tpl_M;
    return r;
}

static FeatureTables feature_tables(const hd_topology* t) {
    const RestraintState& s = t->rs;
    FeatureTables r;
    r.lo = s.ft_lo; r.hi = s.ft_hi; r.k = s.ft_k; r.coef = s.ft_coef; r.sum_f = s.ft_sum;
    r.band_rows = s.ft_band_rows; r.W = s.feat ? s.ft_W : 0; r.sum_rows = s.ft_sum_rows; r.S = s.feat ? s.ft_S : 0;
    r.nv1 = s.ft_nv1; r.nb1 = s.ft_nb1;
    return r;
}

// The restraint part of a path graph's key: all 0 unless the transition is `restrained`; the fields' / templates' generations
// only while some are attached.
static RestraintKey restraint_key(const hd_handle* h, const hd_topology* topo, bool restrained, bool framed) {
    RestraintKey k{};
    if (!restrained) return k;
    const RestraintState& s = topo->rs;
    k.gen = s.gen; k.rows_gen = h->rs_rows.gen; k.frame = framed ? 1 : 0;
    k.fld_gen = s.NF ? s.fld_gen : 0;
    k.tpl_gen = s.NT ? s.tpl_gen : 0;
    k.feat_gen = s.feat ? s.feat_gen : 0;
    return k;
}

// ... and its steering and diversity parts: all 0 unless the term takes part (`on`).
static SteerKey steer_key(const hd_handle* h, const hd_topology* t, bool on) {
    return on ? SteerKey{t->st.P, t->st.ess, t->st.gen, h->st_rows.gen} : SteerKey{};
}
static DiverseKey diverse_key(const hd_handle* h, const hd_topology* t, bool on) {
    return on ? DiverseKey{t->dv.P, t->dv.gen, h->dv_rows.gen} : DiverseKey{};
}

// A transition's row of W floats in the argument struct of any term: the device table `rows` at *io.step / io.row, or the host `row`.
template <typename Args>
static void set_row(Args& a, const LoopIO& io, const float* rows, const float* row, int W) {
    a.rows = rows; a.step_ptr = io.step; a.k = io.row;
    for (int i = 0; i < W; ++i) a.row[i] = row ? row[i] : 0.f;
}

// The update of one transition on eps (in place when out == eps): the row as set_row finds it.  `framed`: in the frame of the known
// fragments io.fixed / io.known (k_restrain_eps<true>).
static int restrain_launch(hd_handle* h, hd_topology* t, const LoopIO& io, const float* z, const float* eps, float* out,
                           const float* rows, const float* row4, bool framed = false) {
    ProfScope ps(h, io.s, 2);
    RestrainArgs a;
    a.z = z; a.eps = eps; a.out = out; a.nm = t->nm_bytes; a.t = restraint_tables(t); a.scale = t->rs.scale;
    set_row(a, io, rows, row4, 4);
    a.step = t->rs.step; a.nv0 = t->rs.nv0; a.scale_rows = t->rs.scale_rows;
    a.B = t->B; a.N = t->N; a.D = h->D;
    a.fixed = framed ? io.fixed : nullptr; a.known = framed ? io.known : nullptr;
    a.tp = template_tables(t);
    const size_t lds = (size_t)t->N * 3 * sizeof(float);
    if (t->rs.NT) {                                     // templates attached: the instantiations with the fit
        if (framed) hipLaunchKernelGGL((k_restrain_eps<true, true>), dim3(t->B), dim3(256), lds, io.s, a);
        else hipLaunchKernelGGL((k_restrain_eps<false, true>), dim3(t->B), dim3(256), lds, io.s, a);
    } else if (framed) hipLaunchKernelGGL((k_restrain_eps<true, false>), dim3(t->B), dim3(256), lds, io.s, a);
    else hipLaunchKernelGGL((k_restrain_eps<false, false>), dim3(t->B), dim3(256), lds, io.s, a);
    HIP_TRY(hipGetLastError());
    return HD_OK;
}

// The feature update of one transition on eps (in place when out == eps), behind restrain_launch: k_restrain_feat on the attached
// features, the row read as there.
static int restrain_feat_launch(hd_handle* h, hd_topology* t, const LoopIO& io, const float* z, const float* eps, float* out,
                                const float* rows, const float* row4) {
    ProfScope ps(h, io.s, 2);
    RestrainFeatArgs a;
    a.z = z; a.eps = eps; a.out = out; a.nm = t->nm_bytes; a.t = feature_tables(t); a.scale = t->rs.scale;
    set_row(a, io, rows, row4, 4);
    a.ratio = t->rs.ft_ratio; a.scale_rows = t->rs.scale_rows;
    a.B = t->B; a.N = t->N; a.D = h->D;
    hipLaunchKernelGGL(k_restrain_feat, dim3(t->B), dim3(256), (size_t)t->N * (h->D - 3) * sizeof(float), io.s, a);
    HIP_TRY(hipGetLastError());
    return HD_OK;
}

// What every entry point that reads the attached restraints refuses first.  `given`: its tensors are there; `templates`: it needs some.
static int restraint_refusals(const char* who, const hd_handle* h, const hd_topology* topo, bool given, const char* what,
                              bool templates = false) {
    if (!h || !topo) return refuse(HD_E_INVALID, who, ": null handle/topology");
    if (!given) return refuse(HD_E_INVALID, who, std::string(": null ") + what);
    if (!topo->rs.on) return refuse(HD_E_STATE, who, ": no restraints attached to the topology (hd_restraint_attach)");
    if (templates && !topo->rs.NT) return refuse(HD_E_STATE, who, ": no templates attached to the topology (hd_restraint_templates)");
    return HD_OK;
}

// ... and the rest of the preamble of the energy entry points: the device, and `stream` behind the arrival of the topology's tables.
static int restraint_entry(const char* who, hd_handle* h, hd_topology* topo, bool given, bool templates, void* stream) {
    HD_TRY(restraint_refusals(who, h, topo, given, "tensor", templates));
    HIP_TRY(hipSetDevice(h->device));
    topo_use(topo, (hipStream_t)stream);
    return HD_OK;
}

// What the single-transition entry points of the eps terms share behind their own state checks; xh_known: framed calls only.
static int eps_entry(const char* who, hd_handle* h, hd_topology* topo, const float* z, const float* eps, const float* row4,
                     const float* xh_known, const float* out, void* stream, LoopIO* io) {
    if (!restraint_row_ok(row4)) return refuse(HD_E_INVALID, who, ": need alpha_t > 0, sigma_t >= 0, a finite lambda and clip > 0 (inf: no clip)");
    const size_t per = (size_t)topo->B * topo->N * h->D;
    if (out < z + per && z < out + per) return refuse(HD_E_INVALID, who, ": out may not overlap z");
    if (xh_known && out < xh_known + per && xh_known < out + per) return refuse(HD_E_INVALID, who, ": out may not overlap xh_known");
    if (out != eps && out < eps + per && eps < out + per) return refuse(HD_E_INVALID, who, ": out may be eps itself, not a shifted overlap of it");
    HIP_TRY(hipSetDevice(h->device));
    *io = LoopIO{}; io->s = (hipStream_t)stream;
    topo_use(topo, io->s);
    return HD_OK;
}

// hd_restrain_eps / hd_restrain_eps_framed (`framed`: fixed_mask and xh_known are part of the call, else null)
static int restrain_eps(const char* who, hd_handle* h, hd_topology* topo, const float* z, const float* eps, const float* row4,
                        const uint8_t* fixed_mask, const float* xh_known, float* out, void* stream, bool framed) {
    HD_TRY(restraint_refusals(who, h, topo, z && eps && row4 && out && (!framed || (fixed_mask && xh_known)),
                              framed ? "tensor / row / fixed_mask / xh_known" : "tensor / row"));
    LoopIO io;
    HD_TRY(eps_entry(who, h, topo, z, eps, row4, xh_known, out, stream, &io));
    io.fixed = fixed_mask; io.known = xh_known;
    return restrain_launch(h, topo, io, z, eps, out, nullptr, row4, framed);
}

extern "C" int hd_restrain_eps(hd_handle* h, hd_topology* topo, const float* z, const float* eps, const float* row4, float* out,
                               void* stream) {
    return restrain_eps("hd_restrain_eps", h, topo, z, eps, row4, nullptr, nullptr, out, stream, false);
}

extern "C" int hd_restrain_feat(hd_handle* h, hd_topology* topo, const float* z, const float* eps, const float* row4, float* out,
                                void* stream) {
    const char* who = "hd_restrain_feat";
    HD_TRY(restraint_refusals(who, h, topo, z && eps && row4 && out, "tensor / row"));
    if (!topo->rs.feat) return refuse(HD_E_STATE, who, ": no features attached to the topology (hd_restraint_features)");
    LoopIO io;
    HD_TRY(eps_entry(who, h, topo, z, eps, row4, nullptr, out, stream, &io));
    return restrain_feat_launch(h, topo, io, z, eps, out, nullptr, row4);
}

extern "C" int hd_restraint_feature_energy(hd_handle* h, hd_topology* topo, const float* hf, double* out2, double* sums, void* stream) {
    const char* who = "hd_restraint_feature_energy";
    HD_TRY(restraint_refusals(who, h, topo, hf && out2, "tensor"));
    if (!topo->rs.feat) return refuse(HD_E_STATE, who, ": no features attached to the topology (hd_restraint_features)");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    topo_use(topo, s);
    ProfScope ps(h, s, 2);
    FeatureEnergyArgs a{};
    a.h = hf; a.nm = topo->nm_bytes; a.t = feature_tables(topo); a.out = out2; a.sums = sums; a.B = topo->B; a.N = topo->N; a.F = h->D - 3;
    hipLaunchKernelGGL(k_restraint_feature_energy, dim3(topo->B), dim3(256), 0, s, a);
    HIP_TRY(hipGetLastError());
    return HD_OK;
}

extern "C" int hd_restrain_eps_framed(hd_handle* h, hd_topology* topo, const float* z, const float* eps, const float* row4,
                                      const uint8_t* fixed_mask, const float* xh_known, float* out, void* stream) {
    return restrain_eps("hd_restrain_eps_framed", h, topo, z, eps, row4, fixed_mask, xh_known, out, stream, true);
}

// One of the four kernels on RestraintEnergyArgs, behind restraint_entry (unframed: fixed_mask, x_known and shift are null).
static int energy_launch(void (*kernel)(RestraintEnergyArgs), hd_handle* h, hd_topology* topo, const float* x, const uint8_t* fixed_mask,
                         const float* x_known, double* out, double* shift3, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(h, s, 2);
    RestraintEnergyArgs a{};
    a.x = x; a.nm = topo->nm_bytes; a.t = restraint_tables(topo); a.out = out; a.B = topo->B; a.N = topo->N;
    a.fixed = fixed_mask; a.x_known = x_known; a.shift = shift3;
    hipLaunchKernelGGL(kernel, dim3(topo->B), dim3(256), 0, s, a);
    HIP_TRY(hipGetLastError());
    return HD_OK;
}

extern "C" int hd_restraint_energy(hd_handle* h, hd_topology* topo, const float* x, double* out3, void* stream) {
    HD_TRY(restraint_entry("hd_restraint_energy", h, topo, x && out3, false, stream));
    return energy_launch(k_restraint_energy<false>, h, topo, x, nullptr, nullptr, out3, nullptr, stream);
}

extern "C" int hd_restraint_energy_framed(hd_handle* h, hd_topology* topo, const float* x, const uint8_t* fixed_mask,
                                          const float* x_known, double* out3, double* shift3, void* stream) {
    HD_TRY(restraint_entry("hd_restraint_energy_framed", h, topo, x && out3 && fixed_mask && x_known, false, stream));
    return energy_launch(k_restraint_energy<true>, h, topo, x, fixed_mask, x_known, out3, shift3, stream);
}

extern "C" int hd_restraint_field_energy(hd_handle* h, hd_topology* topo, const float* x, double* out, void* stream) {
    HD_TRY(restraint_entry("hd_restraint_field_energy", h, topo, x && out, false, stream));
    return energy_launch(k_restraint_field_energy<false>, h, topo, x, nullptr, nullptr, out, nullptr, stream);
}

extern "C" int hd_restraint_field_energy_framed(hd_handle* h, hd_topology* topo, const float* x, const uint8_t* fixed_mask,
                                                const float* x_known, double* out, double* shift3, void* stream) {
    HD_TRY(restraint_entry("hd_restraint_field_energy_framed", h, topo, x && out && fixed_mask && x_known, false, stream));
    return energy_launch(k_restraint_field_energy<true>, h, topo, x, fixed_mask, x_known, out, shift3, stream);
}

extern "C" int hd_restraint_template_energy(hd_handle* h, hd_topology* topo, const float* x, double* out, double* fit16, void* stream) {
    HD_TRY(restraint_entry("hd_restraint_template_energy", h, topo, x && out, true, stream));
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(h, s, 2);
    TemplateEnergyArgs a{};
    a.x = x; a.nm = topo->nm_bytes; a.tp = template_tables(topo); a.out = out; a.fit16 = fit16; a.B = topo->B; a.N = topo->N;
    hipLaunchKernelGGL(k_restraint_template_energy, dim3(topo->B), dim3(256), 0, s, a);
    HIP_TRY(hipGetLastError());
    return HD_OK;
}

// ----------------------------------------------------------------------------- steering: particle resampling on the restraint energy

extern "C" int hd_set_steer(hd_handle* h, int K, const float* rows3) {
    HD_TRY(row_table_check("hd_set_steer", h, K, rows3, 3, steer_row_ok, ": need alpha_t > 0, sigma_t >= 0 and a finite beta_k >= 0"));
    return set_row_table(h, h->st_rows, K, rows3, 3);
}

static SteerState steer_state(const hd_topology* t) {
    SteerState s;
    const size_t B = (size_t)t->B;
    s.logw = t->st.f64; s.uprev = t->st.f64 + B; s.stats = t->st.f64 + 3 * B; s.root = t->st.i32; s.anc = t->st.i32 + B;
    return s;
}

extern "C" int hd_steer_attach(hd_topology* topo, int P, double ess, int reset, void* stream) {
    if (!topo) return fail(HD_E_INVALID, "hd_steer_attach: null topology");
    if (P < 2 || P > ST_MAX_P) return fail(HD_E_INVALID, "hd_steer_attach: need 2 <= P <= 256 particles per group");
    if (topo->B % P != 0) return fail(HD_E_INVALID, "hd_steer_attach: the topology's B is not a multiple of P");
    if (!(ess > 0.0) || !(ess <= 1.0)) return fail(HD_E_INVALID, "hd_steer_attach: need 0 < ess <= 1");
    HIP_TRY(hipSetDevice(topo->device));
    hipStream_t s = (hipStream_t)stream;
    topo_use(topo, s);
    topo->st.on = false;
    const size_t B = (size_t)topo->B;
    const bool fresh = !topo->st.f64;
    if (!reset && (fresh || P != topo->st.P))
        return fail(HD_E_STATE, "hd_steer_attach: reset = 0 continues a chain, and this topology holds no steering state for this P");
    if (fresh) {                                            // all three or none: moved in once every allocation succeeded
        DevBuf<int> i32;
        DevBuf<float> scratch;
        DevBuf<double> f64;
        HD_TRY(i32.alloc(2 * B));
        HD_TRY(scratch.alloc(3 * B * topo->N * topo->h->D));
        HD_TRY(f64.alloc(6 * B));
        topo->st.i32 = std::move(i32); topo->st.scratch = std::move(scratch); topo->st.f64 = std::move(f64);
    }
    if (fresh || P != topo->st.P || ess != topo->st.ess) topo->st.gen++;
    topo->st.P = P; topo->st.ess = ess;
    if (reset) {
        hipLaunchKernelGGL(k_steer_init, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, steer_state(topo), topo->B, P);
        HIP_TRY(hipGetLastError());
    }
    topo->st.on = true;
    return HD_OK;
}

extern "C" int hd_steer_detach(hd_topology* topo) { if (topo) topo->st.on = false; return HD_OK; }

// The three stages of one transition on z / eps (both may be rewritten): `rows` the device table read at *io.step / io.row, or the
// host row; the draw and the first sample id by value or from the loop's device words.
// `hist`: the data prediction the stochastic multistep rows keep, which follows its lineage with z and eps (null: none).
static int steer_launch(hd_handle* h, hd_topology* t, const LoopIO& io, float* z, float* eps, const float* rows, const float* row3,
                        LoopIO::Draw d, uint64_t seed, float* hist = nullptr) {
    ProfScope ps(h, io.s, 2);
    const SteerState st = steer_state(t);
    SteerWeighArgs w;
    w.z = z; w.eps = eps; w.nm = t->nm_bytes; w.t = restraint_tables(t);
    set_row(w, io, rows, row3, 3);
    w.nv0 = t->rs.nv0; w.logw = st.logw; w.uprev = st.uprev; w.B = t->B; w.N = t->N; w.D = h->D;
    w.tp = template_tables(t);
    w.ft = feature_tables(t);
    if (t->rs.feat) {                                   // features attached: the instantiations with U_feat, and v behind x^0 in LDS
        const size_t lds = (size_t)t->N * h->D * sizeof(float);
        if (t->rs.NT) hipLaunchKernelGGL((k_steer_weigh<true, true>), dim3(t->B), dim3(256), lds, io.s, w);
        else hipLaunchKernelGGL((k_steer_weigh<false, true>), dim3(t->B), dim3(256), lds, io.s, w);
    } else if (t->rs.NT) hipLaunchKernelGGL((k_steer_weigh<true, false>), dim3(t->B), dim3(256), (size_t)t->N * 3 * sizeof(float), io.s, w);
    else hipLaunchKernelGGL((k_steer_weigh<false, false>), dim3(t->B), dim3(256), (size_t)t->N * 3 * sizeof(float), io.s, w);
    SteerResampleArgs r;
    r.st = st; r.ess = t->st.ess; r.seed = seed; r.base = io.base; r.draw = d.value; r.draw_ptr = d.word; r.base_ptr = io.base_w;
    r.P = t->st.P;
    hipLaunchKernelGGL(k_steer_resample, dim3(t->B / t->st.P), dim3(256), 0, io.s, r);
    SteerGatherArgs g;
    g.z = z; g.eps = eps; g.hist = hist; g.scratch = t->st.scratch; g.uprev = st.uprev; g.us = t->st.f64 + 2 * (size_t)t->B; g.anc = st.anc;
    g.B = t->B; g.total = t->N * h->D;
    hipLaunchKernelGGL(k_steer_gather<0>, dim3(t->B), dim3(256), 0, io.s, g);
    hipLaunchKernelGGL(k_steer_gather<1>, dim3(t->B), dim3(256), 0, io.s, g);
    HIP_TRY(hipGetLastError());
    return HD_OK;
}

extern "C" int hd_steer_step(hd_handle* h, hd_topology* topo, float* z, float* eps, const float* row3, uint32_t draw, uint64_t seed,
                             uint64_t sample_id_base, void* stream) {
    if (!h || !topo) return fail(HD_E_INVALID, "hd_steer_step: null handle/topology");
    if (!z || !eps || !row3) return fail(HD_E_INVALID, "hd_steer_step: null tensor / row");
    if (!topo->st.on) return fail(HD_E_STATE, "hd_steer_step: no steering attached to the topology (hd_steer_attach)");
    if (!topo->rs.on) return fail(HD_E_STATE, "hd_steer_step: no restraints attached to the topology (hd_restraint_attach)");
    if (!steer_row_ok(row3)) return fail(HD_E_INVALID, "hd_steer_step: need alpha_t > 0, sigma_t >= 0 and a finite beta >= 0");
    const size_t per = (size_t)topo->B * topo->N * h->D;
    if (z < eps + per && eps < z + per) return fail(HD_E_INVALID, "hd_steer_step: z and eps may not overlap");
    HIP_TRY(hipSetDevice(h->device));
    LoopIO io{};
    io.base = sample_id_base; io.s = (hipStream_t)stream;
    topo_use(topo, io.s);
    return steer_launch(h, topo, io, z, eps, nullptr, row3, LoopIO::Draw{draw, nullptr}, seed);
}

extern "C" int hd_steer_read(hd_topology* topo, double* logw, double* uprev, int* root, int* anc, double* stats, void* stream) {
    if (!topo) return fail(HD_E_INVALID, "hd_steer_read: null topology");
    if (!topo->st.f64) return fail(HD_E_STATE, "hd_steer_read: the topology holds no steering state (hd_steer_attach)");
    HIP_TRY(hipSetDevice(topo->device));
    hipStream_t s = (hipStream_t)stream;
    topo_use(topo, s);
    const SteerState st = steer_state(topo);
    const size_t B = (size_t)topo->B;
    if (logw) HIP_TRY(hipMemcpyAsync(logw, st.logw, B * sizeof(double), hipMemcpyDefault, s));
    if (uprev) HIP_TRY(hipMemcpyAsync(uprev, st.uprev, B * sizeof(double), hipMemcpyDefault, s));
    if (root) HIP_TRY(hipMemcpyAsync(root, st.root, B * sizeof(int), hipMemcpyDefault, s));
    if (anc) HIP_TRY(hipMemcpyAsync(anc, st.anc, B * sizeof(int), hipMemcpyDefault, s));
    if (stats) HIP_TRY(hipMemcpyAsync(stats, st.stats, B / topo->st.P * 3 * sizeof(double), hipMemcpyDefault, s));
    return HD_OK;
}

// ----------------------------------------------------------------------------- diversity: rows of a group repel by aligned RMSD

extern "C" int hd_set_diversity(hd_handle* h, int K, const float* rows4) {
    HD_TRY(row_table_check("hd_set_diversity", h, K, rows4, 4, restraint_row_ok,
                           ": need alpha_t > 0, sigma_t >= 0, a finite lambda_k and clip_k > 0 (inf: no clip)"));
    return set_row_table(h, h->dv_rows, K, rows4, 4);
}

// dynamic LDS of k_diverse_eps: x^0 of a group's rows, then - 8-byte aligned - the pair records
static size_t diverse_lds(int P, int N) {
    return (((size_t)P * N * 3 + 1) / 2 + (size_t)P * (P - 1) / 2 * DV_REC) * sizeof(double);
}

extern "C" int hd_diversity_attach(hd_topology* topo, int P, double kappa, double length, const float* scale, int scale_rows, float nv0,
                                   void* stream) {
    const char* who = "hd_diversity_attach";
    if (!topo) return refuse(HD_E_INVALID, who, ": null topology");
    if (P < 2 || P > DV_MAX_P) return refuse(HD_E_INVALID, who, ": need 2 <= P <= 32 rows per group");
    if (topo->B % P != 0) return refuse(HD_E_INVALID, who, ": the topology's B is not a multiple of P");
    if (!scale) return refuse(HD_E_INVALID, who, ": null scale");
    if (scale_rows != 1 && scale_rows != topo->B / P) return refuse(HD_E_INVALID, who, ": scale has 1 row (shared) or B / P rows");
    if (!(kappa >= 0.0) || !(kappa - kappa == 0.0)) return refuse(HD_E_INVALID, who, ": kappa must be >= 0 and finite");
    if (!(length > 0.0) || !(length - length == 0.0)) return refuse(HD_E_INVALID, who, ": length must be positive and finite");
    if (!(nv0 > 0.f) || !(nv0 - nv0 == 0.f)) return refuse(HD_E_INVALID, who, ": nv0 must be positive and finite");
    for (int r = 0; r < scale_rows; ++r)
        if (!(scale[r] - scale[r] == 0.f)) return refuse(HD_E_INVALID, who, ": every scale must be finite");
    // the static LDS of k_diverse_eps is DV_MAX_P * 3 doubles
    if (diverse_lds(P, topo->N) + (size_t)DV_MAX_P * 3 * sizeof(double) > 64 * 1024)
        return refuse(HD_E_INVALID, who, ": P * N * 3 floats and P (P - 1) / 2 pair records exceed one workgroup's LDS");
    HIP_TRY(hipSetDevice(topo->device));
    hipStream_t s = (hipStream_t)stream;
    topo_use(topo, s);
    topo->dv.on = false;
    bool moved = false;
    if (!topo->dv.step) { HD_TRY(topo->dv.step.alloc((size_t)topo->B * topo->N * 3)); moved = true; }
    // (a host array: a pageable source is staged before the call returns)
    HD_TRY(topo->dv.scale.fill(scale, (size_t)scale_rows, &moved, s));
    restraint_bake({{&topo->dv.P, P}, {&topo->dv.scale_rows, scale_rows}},
                   moved || kappa != topo->dv.kappa || length != topo->dv.length || nv0 != topo->dv.nv0, &topo->dv.gen);
    topo->dv.kappa = kappa; topo->dv.length = length; topo->dv.nv0 = nv0;
    topo->dv.on = true;
    return HD_OK;
}

extern "C" int hd_diversity_detach(hd_topology* topo) { if (topo) topo->dv.on = false; return HD_OK; }

// The diversity update of one transition on eps (in place when out == eps): the row read as restrain_launch reads it.
static int diverse_launch(hd_handle* h, hd_topology* t, const LoopIO& io, const float* z, const float* eps, float* out,
                          const float* rows, const float* row4) {
    ProfScope ps(h, io.s, 2);
    DiverseArgs a;
    a.z = z; a.eps = eps; a.out = out; a.nm = t->nm_bytes; a.scale = t->dv.scale;
    set_row(a, io, rows, row4, 4);
    a.step = t->dv.step; a.kappa = t->dv.kappa; a.inv_l2 = 1.0 / (t->dv.length * t->dv.length);
    a.nv0 = t->dv.nv0; a.scale_rows = t->dv.scale_rows; a.P = t->dv.P; a.B = t->B; a.N = t->N; a.D = h->D;
    hipLaunchKernelGGL(k_diverse_eps, dim3(t->B / t->dv.P), dim3(256), diverse_lds(t->dv.P, t->N), io.s, a);
    HIP_TRY(hipGetLastError());
    return HD_OK;
}

extern "C" int hd_diverse_eps(hd_handle* h, hd_topology* topo, const float* z, const float* eps, const float* row4, float* out,
                              void* stream) {
    const char* who = "hd_diverse_eps";
    if (!h || !topo) return refuse(HD_E_INVALID, who, ": null handle/topology");
    if (!z || !eps || !row4 || !out) return refuse(HD_E_INVALID, who, ": null tensor / row");
    if (!topo->dv.on) return refuse(HD_E_STATE, who, ": no diversity attached to the topology (hd_diversity_attach)");
    LoopIO io;
    HD_TRY(eps_entry(who, h, topo, z, eps, row4, nullptr, out, stream, &io));
    return diverse_launch(h, topo, io, z, eps, out, nullptr, row4);
}

extern "C" int hd_diversity_energy(hd_handle* h, hd_topology* topo, const float* x, double* phi, double* rmsd, void* stream) {
    const char* who = "hd_diversity_energy";
    if (!h || !topo) return refuse(HD_E_INVALID, who, ": null handle/topology");
    if (!x || !phi) return refuse(HD_E_INVALID, who, ": null tensor");
    if (!topo->dv.on) return refuse(HD_E_STATE, who, ": no diversity attached to the topology (hd_diversity_attach)");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    topo_use(topo, s);
    ProfScope ps(h, s, 2);
    DiverseEnergyArgs a;
    a.x = x; a.nm = topo->nm_bytes; a.phi = phi; a.rmsd = rmsd; a.kappa = topo->dv.kappa;
    a.inv_l2 = 1.0 / (topo->dv.length * topo->dv.length); a.P = topo->dv.P; a.B = topo->B; a.N = topo->N;
    hipLaunchKernelGGL(k_diverse_energy, dim3(topo->B / topo->dv.P), dim3(256), 0, s, a);
    HIP_TRY(hipGetLastError());
    return HD_OK;
}

// ----------------------------------------------------------------------------- correctors: Langevin steps at the departure level

static bool corrector_row_ok(const float* r) { return r[0] >= 0.f && r[0] - r[0] == 0.f && r[1] >= 0.f && r[1] - r[1] == 0.f && r[2] > 0.f; }
static const char* const kCorrectorRowMsg = ": need sigma_t >= 0, a finite q_k >= 0 and g_max_k > 0 (inf: no cap)";

extern "C" int hd_set_corrector(hd_handle* h, int K, const float* rows3) {
    HD_TRY(row_table_check("hd_set_corrector", h, K, rows3, 3, corrector_row_ok, kCorrectorRowMsg));
    return set_row_table(h, h->cr_rows, K, rows3, 3);
}

extern "C" int hd_corrector_attach(hd_topology* topo, int C, int adaptive, void* stream) {
    const char* who = "hd_corrector_attach";
    if (!topo) return refuse(HD_E_INVALID, who, ": null topology");
    if (C < 1 || C > HD_MAX_CORRECTORS) return refuse(HD_E_INVALID, who, ": need 1 <= C <= 8 corrector steps per transition");
    if (adaptive != 0 && adaptive != 1) return refuse(HD_E_INVALID, who, ": adaptive is 0 (mode \"fixed\") or 1 (mode \"snr\")");
    HIP_TRY(hipSetDevice(topo->device));
    topo_use(topo, (hipStream_t)stream);
    topo->cr.on = false;
    HD_TRY(topo->cr.gain.alloc_once((size_t)HD_MAX_CORRECTORS * topo->B));
    topo->cr.C = C; topo->cr.adaptive = adaptive;
    topo->cr.on = true;
    return HD_OK;
}

extern "C" int hd_corrector_detach(hd_topology* topo) { if (topo) topo->cr.on = false; return HD_OK; }

extern "C" int hd_corrector_read(hd_topology* topo, double* gains, void* stream) {
    if (!topo || !gains) return fail(HD_E_INVALID, "hd_corrector_read: null topology / gains");
    if (!topo->cr.gain || topo->cr.C < 1) return fail(HD_E_STATE, "hd_corrector_read: the topology holds no corrector state (hd_corrector_attach)");
    HIP_TRY(hipSetDevice(topo->device));
    hipStream_t s = (hipStream_t)stream;
    topo_use(topo, s);
    HIP_TRY(hipMemcpyAsync(gains, topo->cr.gain, (size_t)topo->cr.C * topo->B * sizeof(double), hipMemcpyDefault, s));
    return HD_OK;
}

static CorrectorKey corrector_key(const hd_handle* h, const hd_topology* t, bool on) {
    return on ? CorrectorKey{t->cr.C, t->cr.adaptive, h->cr_rows.gen} : CorrectorKey{};
}

// One Langevin step z -> out (in place when out == z) on eps: the row as set_row finds it, the draw and the first sample id by value
// (`ns`) or from the loop's device words.
static int langevin_launch(hd_handle* h, hd_topology* t, const LoopIO& io, const float* z, const float* eps, float* out, double* gain,
                           const float* rows, const float* row3, int adaptive, const NoiseSrc& ns, const uint32_t* draw_w) {
    ProfScope ps(h, io.s, 2);
    LangevinArgs a;
    a.z = z; a.eps = eps; a.nm = t->nm_bytes; a.out = out; a.gain = gain;
    set_row(a, io, rows, row3, 3);
    a.noise = ns; a.draw_ptr = draw_w; a.base_ptr = io.base_w; a.adaptive = adaptive;
    a.B = t->B; a.N = t->N; a.D = h->D; a.F = h->F;
    hipLaunchKernelGGL(k_langevin_step, dim3(t->B), dim3(256), (size_t)t->N * h->D * sizeof(float), io.s, a);
    HIP_TRY(hipGetLastError());
    return HD_OK;
}

extern "C" int hd_langevin_step(hd_handle* h, hd_topology* topo, const float* z, const float* eps, const float* row3, int adaptive,
                                const float* raw_x, const float* raw_h, int noise_rows, uint64_t seed, uint64_t sample_id_base,
                                uint32_t draw, float* out, double* gain_out, void* stream) {
    const char* who = "hd_langevin_step";
    if (!h || !topo) return refuse(HD_E_INVALID, who, ": null handle/topology");
    if (!z || !eps || !row3 || !out) return refuse(HD_E_INVALID, who, ": null tensor / row");
    if (!corrector_row_ok(row3)) return refuse(HD_E_INVALID, who, kCorrectorRowMsg);
    if (adaptive != 0 && adaptive != 1) return refuse(HD_E_INVALID, who, ": adaptive is 0 (mode \"fixed\") or 1 (mode \"snr\")");
    if ((raw_x == nullptr) != (raw_h == nullptr)) return refuse(HD_E_INVALID, who, ": raw_x and raw_h go together");
    if (noise_rows != 1 && noise_rows != topo->B) return refuse(HD_E_INVALID, who, ": noise_rows must be 1 or B");
    const size_t per = (size_t)topo->B * topo->N * h->D;
    if (out < eps + per && eps < out + per) return refuse(HD_E_INVALID, who, ": out may not overlap eps");
    if (out != z && out < z + per && z < out + per) return refuse(HD_E_INVALID, who, ": out may be z itself, not a shifted overlap of it");
    if ((size_t)topo->N * h->D * sizeof(float) > 64 * 1024) return refuse(HD_E_INVALID, who, ": N * D floats exceed one workgroup's LDS");
    HIP_TRY(hipSetDevice(h->device));
    LoopIO io{};
    io.s = (hipStream_t)stream;
    topo_use(topo, io.s);
    return langevin_launch(h, topo, io, z, eps, out, gain_out, nullptr, row3, adaptive,
                           make_noise(raw_x, raw_h, noise_rows, seed, sample_id_base, draw, noise_rows == 1 ? 1 : 0), nullptr);
}

// Classifier-free guidance of a path loop: every network call becomes two (context, then ctx_u) and k_guide_combine in place.
struct GuideSrc {
    const float* ctx_u;   // [B,N,C] the null (or any second) context
    const float* w;       // device [w_rows]
    int w_rows;
    float phi;
};

static int guide_launch(hd_handle* h, hd_topology* t, const float* eps_c, const float* eps_u, const float* w, int w_rows, float phi,
                        float* out, hipStream_t s) {
    ProfScope ps(h, s, 2);
    GuideArgs a;
    a.eps_c = eps_c; a.eps_u = eps_u; a.w = w; a.nm = t->nm_bytes; a.out = out; a.rescale = phi; a.w_rows = w_rows;
    a.B = t->B; a.N = t->N; a.D = h->D;
    hipLaunchKernelGGL(k_guide_combine, dim3(t->B), dim3(256), 0, s, a);
    HIP_TRY(hipGetLastError());
    return HD_OK;
}

// the topology's second network output and the library-owned copies of the null context / the scales: one allocation
static int guide_buffers(hd_handle* h, hd_topology* t) {
    if (t->guide_mem) return HD_OK;
    auto pad = [](size_t n) { return (std::max<size_t>(n, 1) + 63) & ~size_t(63); };
    const size_t BN = (size_t)t->B * t->N;
    const size_t n_eps = pad(BN * h->D), n_ctx = pad(BN * (size_t)std::max(1, h->cfg.context_node_nf)), n_w = pad((size_t)t->B);
    HD_TRY(t->guide_mem.alloc(n_eps + n_ctx + n_w));
    t->eps_u = t->guide_mem; t->ctxu_buf = t->eps_u + n_eps; t->wbuf = t->ctxu_buf + n_ctx;
    return HD_OK;
}

// One frame of the topology's sink (hd_chain_attach) from transition io.row: the state z, or with `eps` the data prediction.
static int chain_launch(hd_handle* h, hd_topology* t, const LoopIO& io, const float* eps) {
    ProfScope ps(h, io.s, 2);
    ChainArgs a;
    a.z = io.z; a.eps = eps; a.nm = t->nm_bytes; a.frame_of = h->chain.d_frame; a.alsig = h->chain.d_as;
    a.dst_w = io.captured() ? h->d_chain_dst : nullptr; a.dst = io.captured() ? nullptr : t->chain.dst; a.step_ptr = io.step; a.k = io.row;
    a.nv0 = t->chain.nv0; a.nv1 = t->chain.nv1; a.nb1 = t->chain.nb1; a.B = t->B; a.N = t->N; a.D = h->D;
    if (eps) hipLaunchKernelGGL(k_chain_frame<1>, dim3(t->B), dim3(256), 0, io.s, a);
    else hipLaunchKernelGGL(k_chain_frame<0>, dim3(t->B), dim3(256), 0, io.s, a);
    HIP_TRY(hipGetLastError());
    return HD_OK;
}

// One call of the path loop.  R = 0 is the plain loop, R >= 1 the inpainting one with R rounds per transition; gd != NULL guides either.
// `slot` keeps the captured transition (a recording one goes to the topology's g_chain instead).  `record`: a sink / restraints
// attached to the topology (hd_chain_attach, hd_restraint_attach) take part - one more launch per transition each, the frame behind
// the update of its last round (the state) or between that round's network call and its update (the data prediction).
struct PathCall {
    float* z;
    const float* context;
    int mol_shape, k_lo, k_hi, use_graph;
    const float *raw_x, *raw_h;                // the noise source
    int noise_rows;
    uint64_t seed, sample_id_base;
    const uint8_t* fixed_mask;                 // inpainting: mask, known values, rounds
    const float* xh_known;
    int R;
    hipStream_t s;
    const PathTables* pt;                      // what it runs on
    GraphSlot<PathKey>* slot;
    bool record;
    const GuideSrc* gd;
};

// The ready checks of the loop terms, asked by path_loop_run in this order: what an attachment asks of the call `c` on the tables `pt`
// (`mol`: the rows that are stepped).  `on`: the term takes part - it is attached and the call records; a call it does not fit is refused.
static int loop_fail(int code, const std::string& msg) { return fail(code, "path loop: " + msg); }
static int chain_ready(const hd_handle* h, const hd_topology* topo, const PathCall& c, const PathTables& pt, int mol, bool* on) {
    if (!(*on = c.record && topo->chain.dst != nullptr)) return HD_OK;
    if (!h->chain.d_frame || h->chain.path_gen != pt.gen)
        return loop_fail(HD_E_STATE, "a chain sink is attached but the chain tables are not set for the current path (hd_set_chain)");
    if (h->chain.frames != topo->chain.frames)
        return loop_fail(HD_E_INVALID, "the attached sink holds " + std::to_string(topo->chain.frames) + " frames, the chain tables were set for " +
                                       std::to_string(h->chain.frames));
    if (topo->chain.what == 1 && !h->chain.d_as)
        return loop_fail(HD_E_STATE, "recording the data prediction needs the {alpha_t, sigma_t} rows (hd_set_chain)");
    if (mol != topo->N) return loop_fail(HD_E_INVALID, "a chain sink records whole molecules only (mol_shape < N)");
    return HD_OK;
}

static int restraint_ready(const hd_handle* h, const hd_topology* topo, const PathCall& c, const PathTables& pt, int mol, bool* on) {
    if (!(*on = c.record && topo->rs.on)) return HD_OK;
    const bool framed = topo->rs.frame == 1;
    if (c.R && !framed)
        return loop_fail(HD_E_INVALID, "restraints are attached to the topology, and inpainting takes none (it re-centres on the known fragments: "
                                       "hd_restraint_detach)");
    if (framed && !c.R)
        return loop_fail(HD_E_INVALID, "the restraints are set to the known fragments' frame (hd_restraint_frame), which needs fixed fragments: an "
                                       "inpainting call");
    if (framed && topo->st.on)
        return loop_fail(HD_E_INVALID, "steering is attached to the topology, and restraints in the known fragments' frame take none (hd_steer_detach)");
    if (!h->rs_rows.d || h->rs_rows.path_gen != pt.gen)
        return loop_fail(HD_E_STATE, "restraints are attached but their rows are not set for the current path (hd_set_restraint)");
    if (mol != topo->N) return loop_fail(HD_E_INVALID, "restraints act on whole molecules only (mol_shape < N)");
    return HD_OK;
}

static int steer_ready(const hd_handle* h, const hd_topology* topo, const PathCall& c, const PathTables& pt, int mol, bool* on) {
    if (!(*on = c.record && topo->st.on)) return HD_OK;
    if (!topo->rs.on)
        return loop_fail(HD_E_STATE, "steering is attached to the topology but no restraints are (hd_restraint_attach): it weighs the particles by "
                                     "their restraint energy");
    if (!h->st_rows.d || h->st_rows.path_gen != pt.gen)
        return loop_fail(HD_E_STATE, "steering is attached but its rows are not set for the current path (hd_set_steer)");
    if (pt.form == 2)
        return loop_fail(HD_E_INVALID, "steering needs a stochastic update, and multistep rows draw nothing (duplicated particles would never "
                                       "diverge: hd_steer_detach)");
    if (c.noise_rows != topo->B) return loop_fail(HD_E_INVALID, "steering needs every row's own noise (noise_rows must be B)");
    return HD_OK;
}

static int diverse_ready(const hd_handle* h, const hd_topology* topo, const PathCall& c, const PathTables& pt, int mol, bool* on) {
    if (!(*on = c.record && topo->dv.on)) return HD_OK;
    if (c.R) return loop_fail(HD_E_INVALID, "diversity is attached to the topology, and inpainting takes none (hd_diversity_detach)");
    if (mol != topo->N) return loop_fail(HD_E_INVALID, "diversity acts on whole molecules only (mol_shape < N)");
    if (topo->st.on)
        return loop_fail(HD_E_INVALID, "diversity and steering are both attached to the topology: a call takes one of them (hd_steer_detach / "
                                       "hd_diversity_detach)");
    if (!h->dv_rows.d || h->dv_rows.path_gen != pt.gen)
        return loop_fail(HD_E_STATE, "diversity is attached but its rows are not set for the current path (hd_set_diversity)");
    if (c.noise_rows == 1)
        for (int k = c.k_lo; k < c.k_hi; ++k)
            if (pt.noisy_h[(size_t)k])
                return loop_fail(HD_E_INVALID, "diversity with one shared row of noise is allowed only on rows that draw nothing (noise_rows must be "
                                               "B on a stochastic path)");
    return HD_OK;
}

static int corrector_ready(const hd_handle* h, const hd_topology* topo, const PathCall& c, const PathTables& pt, int mol, bool* on) {
    if (!(*on = c.record && topo->cr.on)) return HD_OK;
    if (c.R) return loop_fail(HD_E_INVALID, "correctors are attached to the topology, and inpainting takes none (the replacement would have to be "
                                            "redone behind every corrector step: hd_corrector_detach)");
    if (topo->st.on)
        return loop_fail(HD_E_INVALID, "correctors and steering are both attached to the topology: a call takes one of them (hd_steer_detach / "
                                       "hd_corrector_detach)");
    if (mol != topo->N) return loop_fail(HD_E_INVALID, "correctors act on whole molecules only (mol_shape < N)");
    if (c.raw_x) return loop_fail(HD_E_INVALID, "correctors take no injected noise: its K + 2 rows hold none for them (counter-based generator only)");
    if (!h->cr_rows.d || h->cr_rows.path_gen != pt.gen)
        return loop_fail(HD_E_STATE, "correctors are attached but their rows are not set for the current path (hd_set_corrector)");
    return HD_OK;
}

static int path_loop_run(hd_handle* h, hd_topology* topo, const PathCall& c) {
    const PathTables& pt = *c.pt;
    const GuideSrc* gd = c.gd;
    const int T = h->T, K = pt.K, N = topo->N, form = pt.form, R = c.R, k_lo = c.k_lo;
    const int mol = (c.mol_shape < 0 || c.mol_shape > N) ? N : c.mol_shape;
    const int ms = c.mol_shape < 0 ? -1 : mol;
    const uint32_t stride = (uint32_t)T + 2u;
    const int share = (c.noise_rows == 1) ? 1 : 0;
    const int ntr = c.k_hi - k_lo;
    topo_use(topo, c.s);
    if (ntr == 0) return HD_OK;
    if (gd) HD_TRY(guide_buffers(h, topo));
    bool rec, rsn, stn, dvn, crn;                            // which terms take part: one ready check each, in this order
    HD_TRY(chain_ready(h, topo, c, pt, mol, &rec));
    HD_TRY(restraint_ready(h, topo, c, pt, mol, &rsn));
    HD_TRY(steer_ready(h, topo, c, pt, mol, &stn));
    HD_TRY(diverse_ready(h, topo, c, pt, mol, &dvn));
    HD_TRY(corrector_ready(h, topo, c, pt, mol, &crn));
    const int nc = crn ? topo->cr.C : 0;                     // corrector steps per transition, on noise streams 1 .. nc
    const int nd = crn ? 1 + nc : 3 * R;                     // draw words of a captured transition (a corrected call never inpaints)
    const bool framed = rsn && topo->rs.frame == 1;
    const uint8_t* parts = (R && topo->ip_parts_on) ? topo->ip_parts : nullptr;      // calls that do not inpaint ignore the attachment
    const int rounds = R ? R : 1;
    auto score = [&](const LoopIO& io) -> int {              // eps^ of io.z at the departure level, with every eps term in it
        HD_TRY(forward_impl(h, topo, io.z, io.tcur, 1, io.ctx, ms, topo->eps, io.s));
        if (gd) {
            HD_TRY(forward_impl(h, topo, io.z, io.tcur, 1, io.ctx_u, ms, topo->eps_u, io.s));
            HD_TRY(guide_launch(h, topo, topo->eps, topo->eps_u, io.w, gd->w_rows, gd->phi, topo->eps, io.s));
        }
        if (rsn) HD_TRY(restrain_launch(h, topo, io, io.z, topo->eps, topo->eps, h->rs_rows.d, nullptr, framed));
        if (rsn && topo->rs.feat) HD_TRY(restrain_feat_launch(h, topo, io, io.z, topo->eps, topo->eps, h->rs_rows.d, nullptr));
        if (dvn) HD_TRY(diverse_launch(h, topo, io, io.z, topo->eps, topo->eps, h->dv_rows.d, nullptr));
        return HD_OK;
    };
    auto transition = [&](const LoopIO& io) -> int {         // all rounds of one transition; io.row is the path position
        for (int ci = 0; ci < nc; ++ci) {                    // the correctors: Langevin steps on z at the departure level
            HD_TRY(score(io));
            const LoopIO::Draw d = io.draw_of(1 + ci, stride);
            HD_TRY(langevin_launch(h, topo, io, io.z, topo->eps, io.z, topo->cr.gain + (size_t)ci * topo->B, h->cr_rows.d, nullptr,
                                   topo->cr.adaptive, make_noise(nullptr, nullptr, c.noise_rows, c.seed, io.base, d.value, share), d.word));
        }
        for (int j = 0; j < rounds; ++j) {
            HD_TRY(score(io));
            if (stn) HD_TRY(steer_launch(h, topo, io, io.z, topo->eps, h->st_rows.d, nullptr, io.draw_of(0, stride), c.seed,
                                         form == 3 ? topo->ms_hist : nullptr));
            if (rec && j == rounds - 1 && topo->chain.what == 1) HD_TRY(chain_launch(h, topo, io, topo->eps));
            const LoopIO::Draw d = io.draw_of(3 * j, stride);
            const NoiseSrc ns = make_noise(c.raw_x ? c.raw_x + io.ro * 3 : nullptr, c.raw_h ? c.raw_h + io.ro * h->F : nullptr, c.noise_rows,
                                           c.seed, io.base, d.value, share);
            HD_TRY(step_launch(h, topo, io, form, io.z, topo->eps, pt.d_coef + (size_t)io.row * step_row_width(form), 1, nullptr,
                               topo->ms_hist, topo->ms_hist, ns, d.word, mol, N, k_lo));
            if (R) HD_TRY(inpaint_round(h, topo, io, j, R, stride, c.seed, pt.d_coef_ip));
            if (rec && j == rounds - 1 && topo->chain.what == 0) HD_TRY(chain_launch(h, topo, io, nullptr));
        }
        return HD_OK;
    };
    if (!c.use_graph) {
        LoopIO io{};
        io.z = c.z; io.ctx = c.context; io.fixed = c.fixed_mask; io.known = c.xh_known; io.fixed_h = parts; io.base = c.sample_id_base;
        io.s = c.s;
        if (gd) { io.ctx_u = gd->ctx_u; io.w = gd->w; }
        for (int k = k_lo; k < c.k_hi; ++k) {
            io.row = k; io.tcur = h->d_tau + pt.t_h[k];
            io.ro = (size_t)(k - k_lo) * c.noise_rows * mol; io.draw = (uint32_t)(T - pt.s_h[k]);
            HD_TRY(transition(io));
        }
        return HD_OK;
    }
    // The path position lives in d_step; k_path_advance derives the network time, the coefficient row and the draws from the
    // uploaded tables.
    const size_t BN = (size_t)topo->B * N;
    const size_t zbytes = BN * h->D * sizeof(float);
    const size_t cbytes = BN * h->cfg.context_node_nf * sizeof(float);
    hipStream_t rs;
    HD_TRY(replay_enter(h, c.s, &rs));
    HD_TRY(grow_ipdraw(h, rs, nd));
    if (R) HD_TRY(inpaint_buffers(h, topo));
    PathKey key{};
    key.raw_x = c.raw_x; key.raw_h = c.raw_h; key.has_ctx = c.context ? 1 : 0; key.mol_shape = ms; key.noise_rows = c.noise_rows;
    key.k_lo = c.raw_x ? k_lo : 0; key.resamplings = R; key.seed = c.seed; key.weights_gen = h->weights_gen; key.sched_gen = h->sched_gen;
    key.path_gen = pt.gen; key.ip_gen = nd ? h->ip.gen : 0; key.w_rows = gd ? gd->w_rows : 0; key.phi = gd ? gd->phi : 0.f;
    key.ip_parts = parts ? 1 : 0;
    key.rs = restraint_key(h, topo, rsn, framed); key.st = steer_key(h, topo, stn); key.dv = diverse_key(h, topo, dvn);
    key.cr = corrector_key(h, topo, crn);
    PathWords w;
    w.step = h->d_step; w.draw = h->d_draw; w.t_cur = h->d_tcur; w.base = h->d_base; w.ipdraw = nd ? h->ip.d_draw : nullptr;
    w.tau = h->d_tau; w.t_idx = pt.d_t; w.s_idx = pt.d_s; w.K = K; w.T = T; w.nd = nd; w.stride = stride; w.chain = rec ? h->d_chain_dst : nullptr;
    auto body = [&]() -> int {
        LoopIO io = loop_io_captured(h, nd ? h->ip.d_draw : h->d_draw, rs);
        io.z = topo->zbuf; io.ctx = c.context ? topo->ctxbuf : nullptr; io.fixed = topo->ip_fixed; io.known = topo->ip_known;
        io.fixed_h = parts;
        if (gd) { io.ctx_u = topo->ctxu_buf; io.w = topo->wbuf; }
        HD_TRY(transition(io));
        hipLaunchKernelGGL(k_path_advance, dim3(1), dim3(64), 0, rs, w);
        return HD_OK;
    };
    // the caller's slot (the every-step, the guided and the unguided transition are graphs of their own: such calls on one topology
    // do not evict each other); so is the recording one (either kind), keyed on everything it bakes in but the sink's address
    const GraphExec* gx = &c.slot->exec;
    if (rec) {
        gx = &topo->g_chain.exec;
        const ChainSink& sk = topo->chain;
        HD_TRY(replay_slot(h, rs, topo->g_chain, ChainKey{key, sk.what, sk.nv0, sk.nv1, sk.nb1, h->chain.gen}, body));
    } else {
        HD_TRY(replay_slot(h, rs, *c.slot, key, body));
    }
    HIP_TRY(hipMemcpyAsync(topo->zbuf, c.z, zbytes, hipMemcpyDeviceToDevice, rs));
    if (c.context) HIP_TRY(hipMemcpyAsync(topo->ctxbuf, c.context, cbytes, hipMemcpyDeviceToDevice, rs));
    if (gd) {
        HIP_TRY(hipMemcpyAsync(topo->ctxu_buf, gd->ctx_u, cbytes, hipMemcpyDeviceToDevice, rs));
        HIP_TRY(hipMemcpyAsync(topo->wbuf, gd->w, (size_t)gd->w_rows * sizeof(float), hipMemcpyDeviceToDevice, rs));
    }
    if (R) {
        HIP_TRY(hipMemcpyAsync(topo->ip_fixed, c.fixed_mask, BN, hipMemcpyDeviceToDevice, rs));
        HIP_TRY(hipMemcpyAsync(topo->ip_known, c.xh_known, zbytes, hipMemcpyDeviceToDevice, rs));
    }
    hipLaunchKernelGGL(k_path_state, dim3(1), dim3(64), 0, rs, w, k_lo, (unsigned long long)c.sample_id_base, topo->chain.dst);
    HD_TRY(replay_run(*gx, ntr, rs));
    HIP_TRY(hipMemcpyAsync(c.z, topo->zbuf, zbytes, hipMemcpyDeviceToDevice, rs));
    return replay_leave(h, c.s, rs);
}

// The path loop, with the bookkeeping of multistep rows around it.
static int path_loop(hd_handle* h, hd_topology* topo, const PathCall& c) {
    const PathTables& pt = *c.pt;
    HIP_TRY(hipSetDevice(h->device));
    if ((pt.form != 2 && pt.form != 3) || c.k_hi == c.k_lo) return path_loop_run(h, topo, c);
    // multistep rows: the history x^_{k_lo - 1} is the topology's - a call that starts on a row with c2 != 0 continues the call
    // that left it, on the same path (generation) and at the position where that call ended
    const int mol = (c.mol_shape < 0 || c.mol_shape > topo->N) ? topo->N : c.mol_shape;
    if (c.R) return fail(HD_E_INVALID, "multistep path: inpainting takes ancestral rows only");
    if (pt.c2_h[(size_t)c.k_lo] != 0.f && !(topo->ms_hist && topo->ms_gen == pt.gen && topo->ms_k == c.k_lo))
        return fail(HD_E_STATE, "multistep path: transition k_lo = " + std::to_string(c.k_lo) + " needs the data prediction of transition "
                    "k_lo - 1, which the last call on this topology did not leave (start at a row with c2 = 0, such as k_lo = 0, or "
                    "continue where the last call on the same path ended)");
    if ((size_t)mol * h->D * sizeof(float) > 64 * 1024) return fail(HD_E_INVALID, "multistep path: N * D floats exceed one workgroup's LDS");
    HD_TRY(topo->ms_hist.alloc_once((size_t)topo->B * topo->N * h->D));
    topo->ms_gen = 0;                                        // no history unless the whole range ran
    HD_TRY(path_loop_run(h, topo, c));
    topo->ms_gen = pt.gen; topo->ms_k = c.k_hi;              // stream-ordered behind this call, like z
    return HD_OK;
}

static int path_ready(hd_handle* h, const char* who, int k_lo, int k_hi) {
    if (h->T < 1) return fail(HD_E_STATE, std::string(who) + ": schedule not set (hd_set_schedule)");
    if (h->path.K < 1 || h->path.sched_gen != h->sched_gen)
        return fail(HD_E_STATE, std::string(who) + ": path not set for the current schedule (hd_set_path)");
    if (k_lo < 0 || k_lo > k_hi || k_hi > h->path.K) return fail(HD_E_INVALID, std::string(who) + ": need 0 <= k_lo <= k_hi <= K");
    return HD_OK;
}

// The checks a loop without fixed fragments makes on its noise, context and model arguments (inpaint_args_check is the other kind).
static int plain_args_check(const char* who, const hd_handle* h, const hd_topology* topo, const float* raw_x, const float* raw_h,
                            int noise_rows, int mol_shape, const float* context) {
    const std::string w(who);
    if ((raw_x == nullptr) != (raw_h == nullptr)) return fail(HD_E_INVALID, w + ": raw_x and raw_h go together");
    if (noise_rows != 1 && noise_rows != topo->B) return fail(HD_E_INVALID, w + ": noise_rows must be 1 or B");
    if (h->cfg.context_node_nf > 0 && !context) return fail(HD_E_INVALID, w + ": context required");
    if (!h->cfg.condition_time) return fail(HD_E_INVALID, w + ": needs a time-conditioned model");
    if ((size_t)((mol_shape < 0 || mol_shape > topo->N) ? topo->N : mol_shape) * h->D * sizeof(float) > 64 * 1024)
        return fail(HD_E_INVALID, w + ": N * D floats exceed one workgroup's LDS");
    return HD_OK;
}

// The every-step loops: the path loop on the handle's every-step tables, where step s is position T - 1 - s.  Slots of their own
// and no recording - a sink attached to the topology belongs to the caller's path (hd_set_chain).
extern "C" int hd_sample_loop(hd_handle* h, hd_topology* topo, float* z, const float* context, int mol_shape,
                              int s_hi, int s_lo, const float* raw_x, const float* raw_h, int noise_rows,
                              uint64_t seed, uint64_t sample_id_base, int use_graph, void* stream) {
    HD_TRY(check_ready(h, topo, "hd_sample_loop"));
    if (h->T < 1) return fail(HD_E_STATE, "hd_sample_loop: schedule not set (hd_set_schedule)");
    if (!z) return fail(HD_E_INVALID, "hd_sample_loop: null z");
    if (s_hi > h->T || s_lo < 0 || s_lo > s_hi) return fail(HD_E_INVALID, "hd_sample_loop: need 0 <= s_lo <= s_hi <= T");
    HD_TRY(plain_args_check("hd_sample_loop", h, topo, raw_x, raw_h, noise_rows, mol_shape, context));
    PathCall c{};
    c.z = z; c.context = context; c.mol_shape = mol_shape; c.k_lo = h->T - s_hi; c.k_hi = h->T - s_lo; c.raw_x = raw_x; c.raw_h = raw_h;
    c.noise_rows = noise_rows; c.seed = seed; c.sample_id_base = sample_id_base; c.use_graph = use_graph; c.s = (hipStream_t)stream;
    c.pt = &h->every; c.slot = &topo->g_every;
    return path_loop(h, topo, c);
}

extern "C" int hd_sample_loop_inpaint(hd_handle* h, hd_topology* topo, float* z, const float* context, int mol_shape,
                                      int s_hi, int s_lo, const float* raw_x, const float* raw_h, int noise_rows,
                                      uint64_t seed, uint64_t sample_id_base, int use_graph, const uint8_t* fixed_mask,
                                      const float* xh_known, int resamplings, void* stream) {
    const char* who = "hd_sample_loop_inpaint";
    HD_TRY(check_ready(h, topo, who));
    if (h->T < 1) return fail(HD_E_STATE, "hd_sample_loop_inpaint: schedule not set (hd_set_schedule)");
    if (!h->every.d_coef_ip || h->ip.sched_gen != h->sched_gen)
        return fail(HD_E_STATE, "hd_sample_loop_inpaint: inpainting schedule not set for the current schedule (hd_set_inpaint_schedule)");
    if (!z || !fixed_mask || !xh_known) return fail(HD_E_INVALID, "hd_sample_loop_inpaint: null z / fixed_mask / xh_known");
    if (s_hi > h->T || s_lo < 0 || s_lo > s_hi) return fail(HD_E_INVALID, "hd_sample_loop_inpaint: need 0 <= s_lo <= s_hi <= T");
    HD_TRY(inpaint_args_check(who, h, topo, raw_x, raw_h, noise_rows, mol_shape, resamplings, context, kIpRawMsg, kIpRowsMsg));
    PathCall c{};
    c.z = z; c.context = context; c.mol_shape = -1; c.k_lo = h->T - s_hi; c.k_hi = h->T - s_lo;    // no injected noise
    c.noise_rows = noise_rows; c.seed = seed; c.sample_id_base = sample_id_base; c.use_graph = use_graph; c.s = (hipStream_t)stream;
    c.fixed_mask = fixed_mask; c.xh_known = xh_known; c.R = resamplings; c.pt = &h->every; c.slot = &topo->g_every_ip;
    return path_loop(h, topo, c);
}

extern "C" int hd_sample_path(hd_handle* h, hd_topology* topo, float* z, const float* context, int mol_shape, int k_lo, int k_hi,
                              const float* raw_x, const float* raw_h, int noise_rows, uint64_t seed, uint64_t sample_id_base,
                              int use_graph, void* stream) {
    if (k_lo < 0 || k_lo > k_hi) return fail(HD_E_INVALID, "hd_sample_path: need 0 <= k_lo <= k_hi <= K");
    HD_TRY(check_ready(h, topo, "hd_sample_path"));
    HD_TRY(path_ready(h, "hd_sample_path", k_lo, k_hi));
    if (!z) return fail(HD_E_INVALID, "hd_sample_path: null z");
    HD_TRY(plain_args_check("hd_sample_path", h, topo, raw_x, raw_h, noise_rows, mol_shape, context));
    PathCall c{};
    c.z = z; c.context = context; c.mol_shape = mol_shape; c.k_lo = k_lo; c.k_hi = k_hi; c.raw_x = raw_x; c.raw_h = raw_h;
    c.noise_rows = noise_rows; c.seed = seed; c.sample_id_base = sample_id_base; c.use_graph = use_graph; c.s = (hipStream_t)stream;
    c.pt = &h->path; c.slot = &topo->g_path; c.record = true;
    return path_loop(h, topo, c);
}

extern "C" int hd_sample_path_inpaint(hd_handle* h, hd_topology* topo, float* z, const float* context, int mol_shape, int k_lo,
                                      int k_hi, const float* raw_x, const float* raw_h, int noise_rows, uint64_t seed,
                                      uint64_t sample_id_base, int use_graph, const uint8_t* fixed_mask, const float* xh_known,
                                      int resamplings, void* stream) {
    const char* who = "hd_sample_path_inpaint";
    if (k_lo < 0 || k_lo > k_hi) return fail(HD_E_INVALID, "hd_sample_path_inpaint: need 0 <= k_lo <= k_hi <= K");
    HD_TRY(check_ready(h, topo, who));
    if (topo->rs.on && !topo->rs.frame) return fail(HD_E_INVALID, "hd_sample_path_inpaint: restraints are attached to the topology, and inpainting takes "
                                               "none (it re-centres on the known fragments: hd_restraint_detach)");
    HD_TRY(path_ready(h, who, k_lo, k_hi));
    HD_TRY(inpaint_path_check(who, h, ": ancestral rows only (the path was set with form = 1)"));
    if (!z || !fixed_mask || !xh_known) return fail(HD_E_INVALID, "hd_sample_path_inpaint: null z / fixed_mask / xh_known");
    HD_TRY(inpaint_args_check(who, h, topo, raw_x, raw_h, noise_rows, mol_shape, resamplings, context, kIpRawMsg, kIpRowsMsg));
    PathCall c{};
    c.z = z; c.context = context; c.mol_shape = -1; c.k_lo = k_lo; c.k_hi = k_hi;    // no injected noise
    c.noise_rows = noise_rows; c.seed = seed; c.sample_id_base = sample_id_base; c.use_graph = use_graph; c.s = (hipStream_t)stream;
    c.fixed_mask = fixed_mask; c.xh_known = xh_known; c.R = resamplings; c.pt = &h->path; c.slot = &topo->g_path; c.record = true;
    return path_loop(h, topo, c);
}

// ----------------------------------------------------------------------------- classifier-free guidance

extern "C" int hd_guide_combine(hd_handle* h, hd_topology* topo, const float* eps_c, const float* eps_u, const float* w_dev, int w_rows,
                                float rescale, float* out, void* stream) {
    if (!h || !topo) return fail(HD_E_INVALID, "hd_guide_combine: null handle/topology");
    if (!eps_c || !eps_u || !w_dev || !out) return fail(HD_E_INVALID, "hd_guide_combine: null tensor");
    if (w_rows != 1 && w_rows != topo->B) return fail(HD_E_INVALID, "hd_guide_combine: w_rows must be 1 or B");
    if (!(rescale >= 0.f && rescale <= 1.f)) return fail(HD_E_INVALID, "hd_guide_combine: rescale must lie in [0, 1]");
    const size_t per = (size_t)topo->B * topo->N * h->D;
    if (out < eps_u + per && eps_u < out + per) return fail(HD_E_INVALID, "hd_guide_combine: out may not overlap eps_u");
    if (out != eps_c && out < eps_c + per && eps_c < out + per)
        return fail(HD_E_INVALID, "hd_guide_combine: out may be eps_c itself, not a shifted overlap of it");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    topo_use(topo, s);
    return guide_launch(h, topo, eps_c, eps_u, w_dev, w_rows, rescale, out, s);
}

extern "C" long long hd_guided_graph_builds(const hd_topology* topo) { return topo ? topo->g_guided.builds : -1; }

extern "C" int hd_sample_path_guided(hd_handle* h, hd_topology* topo, float* z, const float* context, const float* context_u,
                                     const float* w_dev, int w_rows, float rescale, int k_lo, int k_hi, const float* raw_x,
                                     const float* raw_h, int noise_rows, uint64_t seed, uint64_t sample_id_base, int use_graph,
                                     const uint8_t* fixed_mask, const float* xh_known, int resamplings, void* stream) {
    const char* who = "hd_sample_path_guided";
    if (k_lo < 0 || k_lo > k_hi) return fail(HD_E_INVALID, "hd_sample_path_guided: need 0 <= k_lo <= k_hi <= K");
    HD_TRY(check_ready(h, topo, who));
    HD_TRY(path_ready(h, who, k_lo, k_hi));
    if (h->cfg.context_node_nf < 1) return fail(HD_E_INVALID, "hd_sample_path_guided: needs a context-conditioned model");
    if (!z || !context || !context_u || !w_dev) return fail(HD_E_INVALID, "hd_sample_path_guided: null z / context / context_u / w");
    if (w_rows != 1 && w_rows != topo->B) return fail(HD_E_INVALID, "hd_sample_path_guided: w_rows must be 1 or B");
    if (!(rescale >= 0.f && rescale <= 1.f)) return fail(HD_E_INVALID, "hd_sample_path_guided: rescale must lie in [0, 1]");
    if (!h->cfg.condition_time) return fail(HD_E_INVALID, "hd_sample_path_guided: needs a time-conditioned model");
    if (fixed_mask) {                                        // the restrictions of hd_sample_path_inpaint
        if (topo->rs.on && !topo->rs.frame) return fail(HD_E_INVALID, "hd_sample_path_guided: restraints are attached to the topology, and inpainting "
                                                   "takes none (it re-centres on the known fragments: hd_restraint_detach)");
        HD_TRY(inpaint_path_check(who, h, ": inpainting takes ancestral rows only (the path was set with form = 1)"));
        if (!xh_known) return fail(HD_E_INVALID, "hd_sample_path_guided: fixed_mask without xh_known");
        // no mol_shape here; context and the time-conditioned model were checked above
        HD_TRY(inpaint_args_check(who, h, topo, raw_x, raw_h, noise_rows, -1, resamplings, context,
                                  ": inpainting takes no injected noise (counter-based generator only)", ": inpainting needs noise_rows = B"));
    } else {
        HD_TRY(plain_args_check(who, h, topo, raw_x, raw_h, noise_rows, -1, context));
    }
    const GuideSrc gd{context_u, w_dev, w_rows, rescale};
    PathCall c{};
    c.z = z; c.context = context; c.mol_shape = -1; c.k_lo = k_lo; c.k_hi = k_hi; c.raw_x = raw_x; c.raw_h = raw_h;      // (both null when inpainting)
    c.noise_rows = noise_rows; c.seed = seed; c.sample_id_base = sample_id_base; c.use_graph = use_graph; c.s = (hipStream_t)stream;
    if (fixed_mask) { c.fixed_mask = fixed_mask; c.xh_known = xh_known; c.R = resamplings; }
    c.pt = &h->path; c.slot = &topo->g_guided; c.record = true; c.gd = &gd;
    return path_loop(h, topo, c);
}

// ----------------------------------------------------------------------------- editing given molecules: start state, slerp

extern "C" int hd_diffuse(hd_handle* h, hd_topology* topo, const float* xh, float alpha, float sigma, const float* raw_x,
                          const float* raw_h, int noise_rows, uint64_t seed, uint64_t sample_id_base, uint32_t draw, int share_rows,
                          float* z, void* stream) {
    if (!h || !topo) return fail(HD_E_INVALID, "hd_diffuse: null handle/topology");
    if (!xh || !z) return fail(HD_E_INVALID, "hd_diffuse: null tensor");
    if ((raw_x == nullptr) != (raw_h == nullptr)) return fail(HD_E_INVALID, "hd_diffuse: raw_x and raw_h go together");
    if (noise_rows != 1 && noise_rows != topo->B) return fail(HD_E_INVALID, "hd_diffuse: noise_rows must be 1 or B");
    if ((size_t)topo->N * h->D * sizeof(float) > 64 * 1024) return fail(HD_E_INVALID, "hd_diffuse: N * D floats exceed one workgroup's LDS");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    topo_use(topo, s);
    ProfScope ps(h, s, 2);
    DiffuseArgs a;
    a.xh = xh; a.nm = topo->nm_bytes; a.z = z;
    a.noise = make_noise(raw_x, raw_h, noise_rows, seed, sample_id_base, draw, share_rows);
    a.draw_ptr = nullptr; a.base_ptr = nullptr; a.alpha = alpha; a.sigma = sigma;
    a.B = topo->B; a.N = topo->N; a.D = h->D; a.F = h->F;
    hipLaunchKernelGGL(k_diffuse, dim3(topo->B), dim3(256), (size_t)topo->N * h->D * sizeof(float), s, a);
    HIP_TRY(hipGetLastError());
    return HD_OK;
}

extern "C" int hd_slerp(hd_handle* h, hd_topology* topo, const float* za, const float* zb, const float* lam_host, int L, float* out,
                        void* stream) {
    if (!h || !topo) return fail(HD_E_INVALID, "hd_slerp: null handle/topology");
    if (!za || !zb || !lam_host || !out) return fail(HD_E_INVALID, "hd_slerp: null tensor");
    if (L < 1) return fail(HD_E_INVALID, "hd_slerp: L must be >= 1");
    const size_t per = (size_t)topo->B * topo->N * h->D;
    for (const float* in : {za, zb})
        if (out < in + per && in < out + per * (size_t)L) return fail(HD_E_INVALID, "hd_slerp: out may not alias za or zb");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    topo_use(topo, s);
    ProfScope ps(h, s, 2);
    SlerpArgs a;
    a.za = za; a.zb = zb; a.nm = topo->nm_bytes; a.out = out; a.B = topo->B; a.N = topo->N; a.D = h->D;
    for (int l0 = 0; l0 < L; l0 += SLERP_CHUNK) {      // the weights ride in the kernel arguments: no host buffer outlives the call
        a.l0 = l0; a.n = std::min(SLERP_CHUNK, L - l0);
        for (int i = 0; i < SLERP_CHUNK; ++i) a.lam[i] = i < a.n ? lam_host[l0 + i] : 0.f;
        hipLaunchKernelGGL(k_slerp, dim3(topo->B, a.n), dim3(256), 0, s, a);
        HIP_TRY(hipGetLastError());
    }
    return HD_OK;
}

// ----------------------------------------------------------------------------- scoring: every term of the variational bound

extern "C" int hd_set_nll_terms(hd_handle* h, int K, const int* t_idx, const float* coef4) {
    if (!h || !t_idx || !coef4 || K < 1) return fail(HD_E_INVALID, "hd_set_nll_terms: bad argument");
    if (h->T < 1) return fail(HD_E_STATE, "hd_set_nll_terms: schedule not set (hd_set_schedule)");
    if (K > h->T) return fail(HD_E_INVALID, "hd_set_nll_terms: more terms than the schedule has steps");
    for (int k = 0; k < K; ++k)
        if (t_idx[k] < 1 || t_idx[k] > h->T) return fail(HD_E_INVALID, "hd_set_nll_terms: need 1 <= t_idx[k] <= T");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());                    // a replay may still read the old tables
    h->nll.sched_gen = 0; h->nll.K = 0;
    h->nll.t_h.assign(t_idx, t_idx + K);
    HD_TRY(dev_upload(h->nll.d_t, h->nll.t_h));
    HD_TRY(dev_upload(h->nll.d_coef, std::vector<float>(coef4, coef4 + (size_t)4 * K)));
    h->nll.K = K;
    h->nll.sched_gen = h->sched_gen;
    h->nll.gen++;                              // captured graphs hold the old table addresses
    return HD_OK;
}

extern "C" long long hd_nll_graph_builds(const hd_topology* topo) { return topo ? topo->g_nll.builds : -1; }

// checks shared by hd_nll_terms and hd_nll_finish, in the order the header documents
static int nll_ready(hd_handle* h, hd_topology* topo, const char* who, const float* raw_x, const float* raw_h, int noise_rows,
                     int mol_shape, const float* context) {
    const std::string w(who);
    if (h->T < 1) return fail(HD_E_STATE, w + ": schedule not set (hd_set_schedule)");
    if (h->nll.K < 1 || h->nll.sched_gen != h->sched_gen)
        return fail(HD_E_STATE, w + ": terms not set for the current schedule (hd_set_nll_terms)");
    if ((raw_x == nullptr) != (raw_h == nullptr)) return fail(HD_E_INVALID, w + ": raw_x and raw_h go together");
    if (noise_rows != topo->B) return fail(HD_E_INVALID, w + ": noise_rows must be B");
    if (mol_shape >= 0 && mol_shape < topo->N) return fail(HD_E_INVALID, w + ": fixed tail rows (mol_shape < N) are not supported");
    if (h->cfg.context_node_nf > 0 && !context) return fail(HD_E_INVALID, w + ": context required");
    if (!h->cfg.condition_time) return fail(HD_E_INVALID, w + ": needs a time-conditioned model");
    if ((size_t)topo->N * h->D * sizeof(float) > 64 * 1024) return fail(HD_E_INVALID, w + ": N * D floats exceed one workgroup's LDS");
    return HD_OK;
}

// z_t of io.xh at term io.row into the topology's zbuf, its noise into nll_eps: `coef` the device rows, or {alpha, sigma} by value.
// `ns` carries the host draw and sample base, io their device words.
static int nll_launch_zt(hd_handle* h, hd_topology* t, const LoopIO& io, const float* coef, float alpha, float sigma, const NoiseSrc& ns,
                         int raw_k0) {
    ProfScope ps(h, io.s, 2);
    NllZtArgs a;
    a.xh = io.xh; a.nm = t->nm_bytes; a.eps = t->nll_eps; a.zt = t->zbuf; a.coef = coef; a.noise = ns; a.step_ptr = io.step;
    a.draw_ptr = io.draw_w; a.base_ptr = io.base_w; a.alpha = alpha; a.sigma = sigma; a.k = io.row; a.raw_k0 = raw_k0;
    a.B = t->B; a.N = t->N; a.D = h->D; a.F = h->F;
    hipLaunchKernelGGL(k_nll_zt, dim3(t->B), dim3(256), (size_t)t->N * h->D * sizeof(float), io.s, a);
    HIP_TRY(hipGetLastError());
    return HD_OK;
}

static int nll_launch_err(hd_handle* h, hd_topology* t, const LoopIO& io) {
    ProfScope ps(h, io.s, 2);
    NllErrArgs a;
    a.eps = t->nll_eps; a.net = t->eps; a.coef = h->nll.d_coef; a.acc = io.acc; a.err = io.err; a.step_ptr = io.step; a.k = io.row;
    a.B = t->B; a.ND = t->N * h->D;
    hipLaunchKernelGGL(k_nll_err, dim3(t->B), dim3(256), 0, io.s, a);
    HIP_TRY(hipGetLastError());
    return HD_OK;
}

extern "C" int hd_nll_terms(hd_handle* h, hd_topology* topo, const float* xh, const float* context, int mol_shape, int k_lo, int k_hi,
                            const float* raw_x, const float* raw_h, int noise_rows, uint64_t seed, uint64_t sample_id_base,
                            int use_graph, double* acc, float* err_terms, void* stream) {
    if (k_lo < 0 || k_lo > k_hi) return fail(HD_E_INVALID, "hd_nll_terms: need 0 <= k_lo <= k_hi <= K");
    HD_TRY(check_ready(h, topo, "hd_nll_terms"));
    HD_TRY(nll_ready(h, topo, "hd_nll_terms", raw_x, raw_h, noise_rows, mol_shape, context));
    if (k_hi > h->nll.K) return fail(HD_E_INVALID, "hd_nll_terms: need 0 <= k_lo <= k_hi <= K");
    if (!xh || !acc) return fail(HD_E_INVALID, "hd_nll_terms: null xh / acc");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const int B = topo->B, N = topo->N, K = h->nll.K, nterms = k_hi - k_lo;
    const size_t BN = (size_t)B * N;
    const size_t zbytes = BN * h->D * sizeof(float);
    const size_t cbytes = BN * h->cfg.context_node_nf * sizeof(float);
    topo_use(topo, s);
    if (nterms == 0) return HD_OK;
    HD_TRY(topo->nll_eps.alloc_once(BN * h->D));
    auto term = [&](const LoopIO& io) -> int {               // io.row is the term's position in the list, io.draw its timestep
        HD_TRY(nll_launch_zt(h, topo, io, h->nll.d_coef, 0.f, 0.f, make_noise(raw_x, raw_h, B, seed, io.base, io.draw, 0), k_lo));
        HD_TRY(forward_impl(h, topo, topo->zbuf, io.tcur, 1, io.ctx, -1, topo->eps, io.s));
        return nll_launch_err(h, topo, io);
    };
    if (!use_graph) {
        LoopIO io{};
        io.xh = xh; io.ctx = context; io.acc = acc; io.err = err_terms; io.base = sample_id_base; io.s = s;
        for (int k = k_lo; k < k_hi; ++k) {
            io.row = k; io.draw = (uint32_t)h->nll.t_h[k]; io.tcur = h->d_tau + h->nll.t_h[k];
            HD_TRY(term(io));
        }
        return HD_OK;
    }
    // The term position lives in d_step; k_nll_advance derives the network time and the draw from the uploaded list.
    hipStream_t rs;
    HD_TRY(replay_enter(h, s, &rs));
    HD_TRY(topo->nll_xh.alloc_once(BN * h->D));
    HD_TRY(topo->nll_acc.alloc_once((size_t)B));
    if (err_terms && topo->nll_err_rows < K) {               // grow the e_t table: a graph that holds the old address goes stale (key)
        HD_TRY(replay_quiesce(h, rs));
        topo->nll_err_rows = 0;
        HD_TRY(topo->nll_err.alloc((size_t)K * B));
        topo->nll_err_rows = K;
    }
    NllKey key;
    key.raw_x = raw_x; key.raw_h = raw_h; key.err = err_terms ? topo->nll_err : nullptr; key.has_ctx = context ? 1 : 0;
    key.k_lo = raw_x ? k_lo : 0; key.seed = seed; key.weights_gen = h->weights_gen; key.sched_gen = h->sched_gen; key.nll_gen = h->nll.gen;
    NllWords w;
    w.step = h->d_step; w.draw = h->d_draw; w.t_cur = h->d_tcur; w.base = h->d_base; w.tau = h->d_tau; w.t_idx = h->nll.d_t; w.K = K;
    HD_TRY(replay_slot(h, rs, topo->g_nll, key, [&]() -> int {
        LoopIO io = loop_io_captured(h, h->d_draw, rs);
        io.xh = topo->nll_xh; io.ctx = context ? topo->ctxbuf : nullptr; io.acc = topo->nll_acc; io.err = err_terms ? topo->nll_err : nullptr;
        HD_TRY(term(io));
        hipLaunchKernelGGL(k_nll_advance, dim3(1), dim3(1), 0, rs, w);
        return HD_OK;
    }));
    HIP_TRY(hipMemcpyAsync(topo->nll_xh, xh, zbytes, hipMemcpyDeviceToDevice, rs));
    if (context) HIP_TRY(hipMemcpyAsync(topo->ctxbuf, context, cbytes, hipMemcpyDeviceToDevice, rs));
    HIP_TRY(hipMemcpyAsync(topo->nll_acc, acc, (size_t)B * sizeof(double), hipMemcpyDeviceToDevice, rs));
    hipLaunchKernelGGL(k_nll_state, dim3(1), dim3(1), 0, rs, w, k_lo, (unsigned long long)sample_id_base);
    HD_TRY(replay_run(topo->g_nll.exec, nterms, rs));
    HIP_TRY(hipMemcpyAsync(acc, topo->nll_acc, (size_t)B * sizeof(double), hipMemcpyDeviceToDevice, rs));
    if (err_terms)
        HIP_TRY(hipMemcpyAsync(err_terms + (size_t)k_lo * B, topo->nll_err + (size_t)k_lo * B, (size_t)nterms * B * sizeof(float),
                               hipMemcpyDeviceToDevice, rs));
    return replay_leave(h, s, rs);
}

extern "C" int hd_nll_finish(hd_handle* h, hd_topology* topo, const float* xh, const float* context, int mol_shape, const float* raw_x,
                             const float* raw_h, int noise_rows, uint64_t seed, uint64_t sample_id_base, int K, const float* consts7,
                             int int_nf, int cont_nf, const double* acc, float* nll, void* stream) {
    HD_TRY(check_ready(h, topo, "hd_nll_finish"));
    HD_TRY(nll_ready(h, topo, "hd_nll_finish", raw_x, raw_h, noise_rows, mol_shape, context));
    if (!xh || !acc || !nll || !consts7) return fail(HD_E_INVALID, "hd_nll_finish: null xh / acc / nll / consts7");
    if (K < 1 || K > h->T) return fail(HD_E_INVALID, "hd_nll_finish: need 1 <= K <= T");
    if (int_nf < 0 || cont_nf < 0 || int_nf + cont_nf > h->F)
        return fail(HD_E_INVALID, "hd_nll_finish: int_nf + cont_nf exceed the feature columns");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    topo_use(topo, s);
    if (h->ev_last_set) HIP_TRY(hipStreamWaitEvent(s, h->ev_last, 0));      // zbuf / eps are the replayed term's workspaces too
    HD_TRY(topo->nll_eps.alloc_once((size_t)topo->B * topo->N * h->D));
    LoopIO io{};
    io.xh = xh; io.s = s;
    HD_TRY(nll_launch_zt(h, topo, io, nullptr, consts7[0], consts7[1], make_noise(raw_x, raw_h, topo->B, seed, sample_id_base, 0, 0), 0));
    HD_TRY(forward_impl(h, topo, topo->zbuf, h->d_tau, 1, context, -1, topo->eps, s));
    ProfScope ps(h, s, 2);
    NllFinishArgs a;
    a.net = topo->eps; a.z0 = topo->zbuf; a.xh = xh; a.eps = topo->nll_eps; a.nm = topo->nm_bytes; a.acc = acc; a.nll = nll;
    a.g0 = consts7[2]; a.gT = consts7[3]; a.scale = (float)h->T / (float)K; a.nv2 = consts7[4]; a.nb2 = consts7[5]; a.log_nv0 = consts7[6];
    a.B = topo->B; a.N = topo->N; a.D = h->D; a.int_nf = int_nf; a.cont_nf = cont_nf;
    hipLaunchKernelGGL(k_nll_finish, dim3(topo->B), dim3(256), 0, s, a);
    HIP_TRY(hipGetLastError());
    return HD_OK;
}

extern "C" int hd_inpaint_decode_fix(hd_handle* h, hd_topology* topo, const uint8_t* fixed_mask, const float* x_known,
                                     const float* h_known, float* x, float* hfeat, void* stream) {
    if (!h || !topo) return fail(HD_E_INVALID, "hd_inpaint_decode_fix: null handle/topology");
    if (topo->h != h) return fail(HD_E_INVALID, "hd_inpaint_decode_fix: topology belongs to another handle");
    if (!fixed_mask || !x_known || !h_known || !x || !hfeat) return fail(HD_E_INVALID, "hd_inpaint_decode_fix: null tensor");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    topo_use(topo, s);
    ProfScope ps(h, s, 2);
    InpaintFixArgs a;
    a.nm = topo->nm_bytes; a.fixed = fixed_mask; a.fixed_h = nullptr; a.x_known = x_known; a.h_known = h_known; a.x = x; a.hfeat = hfeat;
    a.B = topo->B; a.N = topo->N; a.F = h->F;
    hipLaunchKernelGGL(k_inpaint_decode_fix<false>, dim3((topo->B + 3) / 4), dim3(256), 0, s, a);
    HIP_TRY(hipGetLastError());
    return HD_OK;
}

// ----------------------------------------------------------------------------- partial inpainting: positions / feature channels

extern "C" int hd_inpaint_parts(hd_handle* h, hd_topology* topo, const uint8_t* fixed_h, void* stream) {
    if (!h || !topo) return fail(HD_E_INVALID, "hd_inpaint_parts: null handle/topology");
    if (topo->h != h) return fail(HD_E_INVALID, "hd_inpaint_parts: topology belongs to another handle");
    if (!fixed_h) { topo->ip_parts_on = false; return HD_OK; }
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    topo_use(topo, s);
    topo->ip_parts_on = false;
    const size_t n = (size_t)topo->B * topo->N * h->F;      // a topology's shape is fixed: the buffer never moves
    HD_TRY(topo->ip_parts.alloc_once(n));
    if (h->ev_last_set) HIP_TRY(hipStreamWaitEvent(s, h->ev_last, 0));      // a replay on another stream may still read the old bytes
    if (n) HIP_TRY(hipMemcpyAsync(topo->ip_parts, fixed_h, n, hipMemcpyDeviceToDevice, s));
    topo->ip_parts_on = true;
    return HD_OK;
}

extern "C" int hd_inpaint_replace(hd_handle* h, hd_topology* topo, float* z, const uint8_t* fixed_x, const uint8_t* fixed_h,
                                  const float* xh_known, float alpha_s, float sigma_s, uint64_t seed, uint64_t sample_id_base,
                                  uint32_t draw, void* stream) {
    if (!h || !topo) return fail(HD_E_INVALID, "hd_inpaint_replace: null handle/topology");
    if (topo->h != h) return fail(HD_E_INVALID, "hd_inpaint_replace: topology belongs to another handle");
    if (!z || !fixed_x || !xh_known) return fail(HD_E_INVALID, "hd_inpaint_replace: null z / fixed_x / xh_known");
    if ((size_t)topo->N * h->D * sizeof(float) > 64 * 1024) return fail(HD_E_INVALID, "hd_inpaint_replace: N * D floats exceed one workgroup's LDS");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    topo_use(topo, s);
    LoopIO io{};
    io.z = z; io.fixed = fixed_x; io.fixed_h = fixed_h; io.known = xh_known; io.base = sample_id_base; io.s = s;
    const float row[4] = {alpha_s, sigma_s, 0.f, 0.f};
    return inpaint_launch(h, topo, io, false, LoopIO::Draw{draw, nullptr}, seed, nullptr, row);
}

extern "C" int hd_inpaint_decode_fix_parts(hd_handle* h, hd_topology* topo, const uint8_t* fixed_x, const uint8_t* fixed_h,
                                           const float* x_known, const float* h_known, float* x, float* hfeat, void* stream) {
    if (!h || !topo) return fail(HD_E_INVALID, "hd_inpaint_decode_fix_parts: null handle/topology");
    if (topo->h != h) return fail(HD_E_INVALID, "hd_inpaint_decode_fix_parts: topology belongs to another handle");
    if (!fixed_x || !fixed_h || !x_known || !h_known || !x || !hfeat) return fail(HD_E_INVALID, "hd_inpaint_decode_fix_parts: null tensor");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    topo_use(topo, s);
    ProfScope ps(h, s, 2);
    InpaintFixArgs a;
    a.nm = topo->nm_bytes; a.fixed = fixed_x; a.fixed_h = fixed_h; a.x_known = x_known; a.h_known = h_known; a.x = x; a.hfeat = hfeat;
    a.B = topo->B; a.N = topo->N; a.F = h->F;
    hipLaunchKernelGGL(k_inpaint_decode_fix<true>, dim3((topo->B + 3) / 4), dim3(256), 0, s, a);
    HIP_TRY(hipGetLastError());
    return HD_OK;
}
