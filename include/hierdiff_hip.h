/*
 * hierdiff_hip.h -- C ABI of libhierdiff_hip.so: the MI355X (gfx950) implementation of HierDiff's
 * coarse-grained reverse-diffusion hot path (EGNN dynamics forward + posterior step).
 *
 * Every entry point takes plain pointers and sizes; there are no torch / C++ types in the
 * signatures.  Device pointers are raw HIP device addresses (tensor.data_ptr()), `stream` is a
 * hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream), NULL = default stream.
 *
 * Conventions
 *   - return value 0 = OK, negative = error (HD_E_*); the message is in hd_last_error()
 *     (thread-local).  No exceptions or aborts cross the ABI.  Kernel faults surface at the
 *     caller's next synchronisation.
 *   - one handle per (device, stream of use); calls on one handle must be serialised by the
 *     caller; distinct handles are independent: the library keeps no process-global mutable
 *     state besides the thread-local hd_last_error() text.
 *   - the handle OWNS a repacked device copy of the weights; a topology OWNS its index tables
 *     and activation workspace; the caller owns every tensor it passes in.
 *
 * Reference interfaces replaced (file:line under /root/reference/endiffusion):
 *   hd_create / hd_set_weights   <- EGNN_dynamics_QM9.__init__ + load_state_dict
 *                                   (models/module/en_dynamics.py:9-36, sampler.py:27-34)
 *   hd_topology_create           <- get_adj_matrix + the mask tensors built in
 *                                   DiffusionQM9.sample (en_dynamics.py:124-143,
 *                                   train_module/diffusion_qm9.py:350-359)
 *   hd_egnn_forward              <- EGNN_dynamics_QM9._forward (en_dynamics.py:49-122), i.e.
 *                                   DiffusionQM9.phi (diffusion_qm9.py:135-138)
 *   hd_posterior_step            <- the arithmetic of sample_p_zs_given_zt after the network call
 *                                   (diffusion_qm9.py:328-345) incl. sample_normal (:438-456)
 *   hd_final_decode              <- sample_p_xh_given_z0 after the network call (:302-310)
 *   hd_noise                     <- sample_combined_position_feature_noise (:445-456)
 *   hd_sample_loop               <- the timestep loop of DiffusionQM9.sample (:375-384)
 *   hd_sample_loop_inpaint       <- no counterpart: the same loop with known fragments kept in place
 *   hd_sample_path_guided        <- no counterpart: the path loop with classifier-free guidance (two network calls per transition)
 *   hd_nll_terms / hd_nll_finish <- the one-timestep estimator of compute_loss / nll in eval mode (:530-699), every listed t
 */
#ifndef HIERDIFF_HIP_H
#define HIERDIFF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HD_ABI_VERSION 12

#define HD_OK 0
#define HD_E_INVALID (-1)      /* bad argument / unsupported configuration */
#define HD_E_HIP (-2)          /* a HIP runtime call failed */
#define HD_E_NOMEM (-3)
#define HD_E_STATE (-4)        /* e.g. weights or schedule not set */

typedef struct hd_handle hd_handle;
typedef struct hd_topology hd_topology;

/* Mirrors EGNN_dynamics_QM9's constructor arguments (en_dynamics.py:9-13) that are on the path.
 * Unsupported values (mode != egnn_dynamics, sin_embedding, act_fn != silu) are rejected by the Python wrapper
 * before this struct is built. */
typedef struct hd_config {
    int32_t in_node_nf;          /* node features INCLUDING the time column, excluding context */
    int32_t context_node_nf;
    int32_t n_dims;              /* must be 3 */
    int32_t hidden_nf;           /* 32, 64, 128 or 256 (en_dynamics.py:9 accepts any width; production: 256).  Other multiples of 32
                                    are rejected by hd_create, not padded: every kernel is instantiated per width - the edge kernels
                                    keep H/32 accumulators in registers and deal H/32 column tiles to 4 or 8 wavefronts, the chunk
                                    images are cut into 1 KiB pieces per four wavefronts - and a zero-padded 256-wide network would
                                    change the summation order of every contraction, i.e. the bits, of a narrower model */
    int32_t n_layers;            /* number of EquivariantBlocks */
    int32_t inv_sublayers;       /* GCLs per block */
    int32_t attention;           /* 0/1 */
    int32_t tanh;                /* 0/1 */
    int32_t condition_time;      /* 0/1 */
    float norm_constant;
    float normalization_factor;
    float coords_range;          /* EGNN default 30; per-block range = coords_range / n_layers */
    int32_t precision;           /* matrix-core arithmetic of the H x H contractions:
                                    0 = exact fp32 (v_mfma_f32_32x32x2_f32) - what the reference computes in,
                                        and the default of the Python mirror,
                                    3 = "fp16x3" (opt-in): the per-edge contraction on a two-way FP16 split (11 + 11 significant
                                        bits per operand), 3 fp16 MFMAs per product, fp32 accumulation - truncation <= 2^-21 per
                                        product, at the rounding of the fp32 accumulation (measured 1.9e-7 rel-L2 on a 256-term
                                        contraction).  Operands are ranged by exact powers of two - W2 per matrix, the
                                        activations per edge row from a bound on the pre-activation known before the contraction
                                        starts - so FP16's exponent range imposes no assumption on the network.  The node GEMMs
                                        run the same arithmetic (hidden_nf >= 128; narrower: mode 0's node kernels).
                                    1 ("bf16x3") and 2 ("bf16x6") existed up to ABI 11 and are rejected since ABI 12: fp16x3
                                    is as accurate as 2 at the cost of 1 */
    int32_t aggregation_mean;    /* 0: aggregation_method 'sum' - neighbour sums / normalization_factor (egnn_new.py:280-282);
                                    1: 'mean' (:283-288) - sums / number of edge-list entries of the receiving node.  The
                                       reference's edge list holds all N x N pairs of a molecule, masked or not
                                       (en_dynamics.py:124-143), so that count is the padded N of the call for every node
                                       and normalization_factor is unused */
} hd_config;

int hd_version(void);
const char* hd_last_error(void);

/* Number of HIP devices visible (0 when there is no GPU; never fails). */
int hd_device_count(void);

int hd_create(const hd_config* cfg, int device, hd_handle** out);
int hd_destroy(hd_handle* h);

/* Number of fp32 values in the canonical weight blob: the dynamics parameters flattened in
 * state_dict registration order (hierdiff_amd/weights.py::dynamics_param_shapes). */
long long hd_weight_count(const hd_handle* h);

/* Load the canonical weight blob (host or device pointer). The library repacks it into its
 * kernel layouts; the source is not referenced after return. */
int hd_set_weights(hd_handle* h, const float* blob, long long n, int on_device, void* stream);

/* Build index tables for one (node_mask, edge_mask) pair.  Masks are HOST byte arrays
 * (0 = false): node_mask [B*N], edge_mask [B*N*N] row-major (b, i, j) or NULL for the canonical
 * mask node_mask[i] & node_mask[j] & (i != j).  The tables are laid out per molecule, so the bits
 * computed for a molecule do not depend on the rest of the batch (sharding a batch over ranks
 * reproduces the single-GPU result exactly). */
int hd_topology_create(hd_handle* h, const uint8_t* node_mask, const uint8_t* edge_mask, int B, int N,
                       hd_topology** out);
/* The same, without a host wait: the tables travel pinned staging -> device in stream order of `stream` (the workspace
 * fill behind them), so the call returns as soon as the host-side layout is done and a training loop that meets new masks
 * every step keeps the GPU busy while the next batch's topology is laid out.  Launches on the topology from another stream
 * wait for the tables' arrival by themselves.  Device arena and staging buffer come from a grow-only pool that
 * hd_topology_destroy refills (no hipMalloc / hipFree / device-wide synchronisation per topology in steady state). */
int hd_topology_create_s(hd_handle* h, const uint8_t* node_mask, const uint8_t* edge_mask, int B, int N, void* stream,
                         hd_topology** out);
/* Returns the topology's memory to the pool behind an event on the stream it was last used on (a topology that captured
 * a sampling graph or ran on several streams waits for the device instead). */
int hd_topology_destroy(hd_topology* t);
/* Frees every pooled arena (after their pending work). */
int hd_arena_pool_trim(void);
/* The device allocations the library holds in this process, on all devices: what handles, topologies and stage-2 objects own,
 * and the pooled arenas (memory torch's allocator cannot see; memory torch allocated does not count).  `bytes`, if not null,
 * receives their size.  After every object is destroyed and the pool is trimmed both are 0.  Needs no GPU (then: 0). */
long long hd_live_allocations(long long* bytes);
/* Host-only view of the edge-tile tables hd_topology_create builds for the same masks (no device needed): edges are
 * packed in 32-row tiles per molecule - cuts at molecule-relative multiples of 32, remainders of neighbouring
 * molecules share a tile at 4-row-aligned offsets - so the rows summed into one partial sum ("part") of a node
 * depend on its molecule alone.  counts5 = {active nodes, valid edges, tiles, parts, rows = 32 * tiles}; the
 * output arrays may be NULL: ei/ej [rows] receiving/sending compact node id, eseg [rows] segment of the row inside
 * its tile (255 = padding row), seg_part [rows] part id per (tile, segment), tile_nseg [tiles], pstart [nodes+1]
 * (a node's parts are pstart[i] .. pstart[i+1]-1, in the order consumers add them). */
int hd_topology_layout(const uint8_t* node_mask, const uint8_t* edge_mask, int B, int N, long long* counts5,
                       int* ei, int* ej, uint8_t* eseg, int* seg_part, int* tile_nseg, int* pstart);
/* info[0..5] = {B, N, active nodes, valid edges, edge tiles (32 edges), aggregation parts} */
int hd_topology_info(const hd_topology* t, long long* info6);

/* out[B,N,3+F] = EGNN_dynamics_QM9._forward(t, xh, node_mask, edge_mask, context, mol_shape).
 *   xh      device [B,N,3+F], F = in_node_nf - condition_time
 *   t       device, t_numel == 1 (broadcast) or B
 *   context device [B,N,context_node_nf] or NULL when context_node_nf == 0
 *   mol_shape  < 0 for None; otherwise nodes >= mol_shape keep their input coordinates
 * Stream-ordered; the NaN guard (whole-call reset of the velocity, en_dynamics.py:109-111) is
 * applied on the device without a host sync. */
int hd_egnn_forward(hd_handle* h, hd_topology* topo, const float* xh, const float* t, int t_numel,
                    const float* context, int mol_shape, float* out, void* stream);

/* Number of forwards since creation whose velocity contained NaN (syncs the stream). */
int hd_nan_events(hd_handle* h, void* stream, long long* count);

/* zs[B,mol,D] = posterior sample given the network output eps[B,N,D] (diffusion_qm9.py:326-345).
 *   coef   device [B,4] or [1,4] (coef_rows = B or 1): {alpha_t_given_s, sigma2_t_given_s,
 *          sigma_t, sigma = sigma_t_given_s * sigma_s / sigma_t}
 *   raw_x  device [noise_rows, mol, 3], raw_h device [noise_rows, mol, F]: the two randn draws;
 *          noise_rows = 1 reproduces fix_noise=True.  mol = mol_shape (< 0: N).
 *   zs may alias zt only when mol == N.
 * One workgroup per molecule keeps the mol * D values of its molecule in LDS: mol * D * sizeof(float) > 64 KiB is refused on the host,
 * before any launch, with HD_E_INVALID ("hd_posterior_step: N * D floats exceed one workgroup's LDS"), like hd_multistep_step and
 * hd_diffuse.  hd_sample_loop, hd_sample_path and hd_sample_path_guided, which launch the same kernel, refuse it under their own names. */
int hd_posterior_step(hd_handle* h, hd_topology* topo, const float* zt, const float* eps, const float* coef,
                      int coef_rows, const float* raw_x, const float* raw_h, int noise_rows, int mol_shape,
                      float* zs, void* stream);

/* x[B,N,3], hfeat[B,N,F] = sample_p_xh_given_z0 after the network call.
 *   coef3 host {sigma_0, alpha_0, sigma_x}; noise as in hd_noise (raw normals or, with
 *   raw_x == NULL, the counter-based generator at (seed, sample_id_base + b, draw)). */
int hd_final_decode(hd_handle* h, hd_topology* topo, const float* z0, const float* eps, const float* coef3,
                    const float* raw_x, const float* raw_h, int noise_rows, uint64_t seed,
                    uint64_t sample_id_base, uint32_t draw, int share_rows, float* x, float* hfeat,
                    void* stream);

/* z[rows,N,3+F] = masked, centre-of-gravity-free combined noise from raw normals (rows = B), or,
 * with raw_x == NULL, from the library's counter-based generator (Philox4x32-10 + Box-Muller):
 * normal(seed, sample_id_base + b, draw, n*D + c).  share_rows != 0 draws one row (sample id
 * sample_id_base) and broadcasts it over the batch before masking (fix_noise).
 *
 * Draw layout of one sample (seed, sample id): every normal is normal(seed, sample id, draw, n*D + c).
 *   plain sampling        draw 0 = z_T, draw T - s = the posterior step s (t = s + 1), draw T + 1 = the final decode;
 *   inpainting loop       draw = (T + 2) * (3 j + k) + (T - s) for resampling round j = 0 .. r-1 of step s and stream
 *                         k = 0 posterior step, 1 noise of the known part (e_kn), 2 noise of the jump back (e_jump).
 *                         (j, k) = (0, 0) is the plain stream, so r = 1 without fixed nodes reproduces plain sampling bit for bit;
 *                         (T + 2) * 3 r must fit 32 bits.
 *   path loops            (hd_sample_path, hd_sample_path_inpaint) the counter is the FINE-GRID index of the arrival step: the
 *                         transition t -> s of a path draws at T - s (inpainting: (T + 2) * (3 j + k) + (T - s)), draw 0 = z_T and
 *                         draw T + 1 = the final decode as above - the layouts above restricted to the visited s.  The identity path
 *                         T, T-1, .., 0 is what hd_sample_loop / hd_sample_loop_inpaint run on; uploaded through hd_set_path it
 *                         gives their bits.
 *   scoring               (hd_nll_terms, hd_nll_finish) a stream of its own, used with the DATA of a sample instead of its chain: the
 *                         noise eps_t of the bound's term t = 1 .. T is draw = t, the noise eps_0 of the t = 0 likelihood is draw 0.
 *                         The counter is the term's grid index, never its position in the term list, so a molecule's score does not
 *                         depend on the order of the terms or on how their range was split into calls.
 *   editing               (hd_diffuse, then hd_sample_path on a partial path) the start state z_{t_start} = alpha xh + sigma eps draws at
 *                         draw 0, the slot plain sampling uses for z_T; the partial chain below it draws at T - s of the steps it visits
 *                         and the decode at T + 1 - the plain layout with draw 0 re-purposed and draws 1 .. T - t_start unused.
 *                         Inversion (hd_set_path_up) and hd_slerp draw nothing.
 *   guidance              (hd_sample_path_guided, hd_guide_combine) guided loops draw what their unguided loop draws. */
int hd_noise(hd_handle* h, hd_topology* topo, const float* raw_x, const float* raw_h, int noise_rows,
             uint64_t seed, uint64_t sample_id_base, uint32_t draw, int share_rows, float* z, void* stream);

/* Schedule for hd_sample_loop: host arrays of T+1 time values tau[k] = fp32(k)/T and T rows of
 * {alpha_t_given_s, sigma2_t_given_s, sigma_t, sigma} for s = 0..T-1 (t = s+1).  The library keeps them as the handle's built-in
 * every-step tables: the identity path T -> T-1 -> .. -> 0 with these rows, next to and independent of the caller's path
 * (hd_set_path below). */
int hd_set_schedule(hd_handle* h, int T, const float* tau, const float* coef4);

/* Runs posterior steps s = s_hi-1 ... s_lo on z[B,N,D] in place (rows >= mol_shape untouched):
 * per step one hd_egnn_forward at tau[s+1] and one hd_posterior_step.  This is the path loop (hd_sample_path below) on the handle's
 * every-step tables, transitions T - s_hi ... T - s_lo - 1, with a graph slot of its own: it and hd_sample_path do not evict each
 * other, and hd_path_graph_builds does not count it.
 *   raw_x/raw_h  device [(s_hi-s_lo), noise_rows, mol, 3|F] in step order (first = s_hi-1), or NULL
 *                to use the counter-based generator with draw = T - s (draw 0 is z_T).  (The loop on a sub-sequence of the
 *                grid is hd_sample_path below; its draws are the same T - s of the steps it visits.)
 *   use_graph    replay each step from a captured hipGraph (0 = plain launches).  The instantiated graph is
 *                cached with the topology and reused by later calls with the same arguments (any z / context /
 *                sample_id_base); it is stream-ordered like every other call - no host synchronisation.
 * HD_E_INVALID, before any launch: mol * D floats beyond one workgroup's LDS (64 KiB), as hd_posterior_step. */
int hd_sample_loop(hd_handle* h, hd_topology* topo, float* z, const float* context, int mol_shape,
                   int s_hi, int s_lo, const float* raw_x, const float* raw_h, int noise_rows,
                   uint64_t seed, uint64_t sample_id_base, int use_graph, void* stream);

/* ---- Few-step sampling (ABI 12, additive): the reverse chain on a sub-sequence of the schedule's grid.  A path is K transitions
 * t_idx[k] -> s_idx[k] (grid indices, 0 <= s_idx[k] < t_idx[k] <= T, t_idx[k + 1] = s_idx[k]); the update of sample_p_zs_given_zt
 * (diffusion_qm9.py:312-345) holds for any s < t.  hd_set_path uploads the path next to the plain schedule, which must be set (it
 * supplies T and tau) and whose replacement needs a new upload here (HD_E_STATE otherwise).  Host arrays:
 *   coef4          K rows; form 0: {alpha_t_given_s, sigma2_t_given_s, sigma_t, sigma} of (s_idx[k], t_idx[k]), the plain step's row;
 *                  form 1: {a, b, c, 0} of the linear update z_s = (a z_t - b eps) + c noise (DDIM family: sigma~ = eta sigma_t|s sigma_s /
 *                  sigma_t, a = alpha_s / alpha_t, b = a sigma_t - sqrt(sigma_s^2 - sigma~^2), c = sigma~), eps and noise with their x parts
 *                  mean-removed and the result re-centred as in the plain step.  A row with c == 0 generates and reads no normal.
 *   coef4_inpaint  NULL, or K rows {alpha_s, sigma_s, alpha_t_given_s, sigma_t_given_s} for hd_sample_path_inpaint (form 0 only). */
int hd_set_path(hd_handle* h, int K, const int* t_idx, const int* s_idx, const float* coef4, int form, const float* coef4_inpaint);
/* Transitions k = k_lo ... k_hi-1 of the path on z[B,N,D] in place; arguments, stream ordering, pocket rows (mol_shape) and shared
 * noise rows (noise_rows = 1) as in hd_sample_loop.  Network time tau[t_idx[k]]; noise counter T - s_idx[k] (layout at hd_noise).
 *   raw_x/raw_h  device [(k_hi-k_lo), noise_rows, mol, 3|F] indexed by path position (first = k_lo), or NULL.
 *   use_graph    ONE captured transition per topology, whatever K: the path position lives in device memory and the captured
 *                kernels read time, coefficient row and draw through the uploaded tables.  Cached like the plain loop's graph and
 *                rebuilt when the path, seed, weights, schedule or noise arguments change; use_graph = 0 gives the same bits.
 * HD_E_INVALID, before any launch: mol * D floats beyond one workgroup's LDS (64 KiB), as hd_posterior_step. */
int hd_sample_path(hd_handle* h, hd_topology* topo, float* z, const float* context, int mol_shape, int k_lo, int k_hi,
                   const float* raw_x, const float* raw_h, int noise_rows, uint64_t seed, uint64_t sample_id_base,
                   int use_graph, void* stream);
/* hd_sample_loop_inpaint on the path: the rounds 1 - 4 below per transition (s, t) = (s_idx[k], t_idx[k]).  Restrictions of
 * hd_sample_loop_inpaint, and the path must hold ancestral rows (form 1: HD_E_INVALID) and inpainting rows (else HD_E_STATE). */
int hd_sample_path_inpaint(hd_handle* h, hd_topology* topo, float* z, const float* context, int mol_shape, int k_lo, int k_hi,
                           const float* raw_x, const float* raw_h, int noise_rows, uint64_t seed, uint64_t sample_id_base,
                           int use_graph, const uint8_t* fixed_mask, const float* xh_known, int resamplings, void* stream);
/* Number of times the topology's captured path transition was instantiated (-1: null topology): a cached replay leaves it unchanged. */
long long hd_path_graph_builds(const hd_topology* topo);

/* ---- Editing given molecules (ABI 12, additive; no reference counterpart): start a reverse chain from a noised molecule instead of
 * z_T (variations of a lead; the SDEdit idea), run the deterministic eta = 0 update UPWARDS in t to encode a molecule to its latent
 * ("DDIM inversion"), and interpolate latents on the sphere.  Mechanism only: which t_start, K and eta are chemically useful is for
 * the user to validate on a trained checkpoint.
 *
 * hd_diffuse: z[B,N,D] = alpha xh + sigma eps for normalised data xh [B,N,D], eps = the combined noise of hd_noise (masked, x part
 * mean-free over the valid nodes; raw_x / raw_h device [noise_rows,N,3|F] with noise_rows = B or 1 = one shared row, or NULL = the
 * generator at (seed, sample_id_base + b, draw), share_rows as in hd_noise; eps equals hd_noise's tensor for the same arguments bit
 * for bit).  alpha / sigma: sqrt(sigmoid(-+gamma_t)) of the grid point the caller starts from.  sigma == 0 generates and reads no
 * normal (z_0 = alpha_0 xh, the start of an inversion).  Writes z only; a molecule without valid nodes gets alpha xh.  Stream-ordered,
 * no host synchronisation.  HD_E_INVALID: raw_x and raw_h not both given or both NULL, noise_rows not 1 or B, N * D floats beyond one
 * workgroup's LDS (64 KiB). */
int hd_diffuse(hd_handle* h, hd_topology* topo, const float* xh, float alpha, float sigma, const float* raw_x, const float* raw_h,
               int noise_rows, uint64_t seed, uint64_t sample_id_base, uint32_t draw, int share_rows, float* z, void* stream);
/* An ASCENDING path into the tables hd_set_path fills: K transitions from_idx[k] -> to_idx[k] with 0 <= from_idx[k] < to_idx[k] <= T,
 * from_idx[k + 1] = to_idx[k], K <= T (HD_E_INVALID otherwise; hd_set_path itself keeps refusing ascending pairs).  Host rows coef4
 * {a, b, 0, 0} of z_v = (a z_u - b eps) for u = from_idx[k], v = to_idx[k]: a = alpha_v / alpha_u, b = a sigma_u - sigma_v, the eta = 0
 * row of hd_set_path with the roles of s and t exchanged; a non-zero third or fourth entry is HD_E_INVALID - inversion draws nothing.
 * Form 1, no inpainting rows.  The network time of transition k is tau[from_idx[k]], the departure, as for descending paths.
 * hd_sample_path then runs either direction unchanged (one captured transition per topology, the cached graph rebuilt when the path
 * changes); hd_sample_path_inpaint on an ascending path is HD_E_INVALID.  Schedule requirements as hd_set_path. */
int hd_set_path_up(hd_handle* h, int K, const int* from_idx, const int* to_idx, const float* coef4);
/* out[L,B,N,D]: per molecule and weight lam_l (HOST array of L >= 1 floats) the spherical interpolation
 *     out_l = (sin((1 - lam_l) theta) za + sin(lam_l theta) zb) / sin theta,   theta = acos(clamp(<za, zb> / (|za| |zb|), -1, 1)),
 * of two latents za, zb [B,N,D] on the topology's masks; dot product and norms run over the valid entries, accumulated in double in a
 * fixed order, theta and the two weights in double, the combination in fp32.  Where sin theta < 1e-6 (parallel or antiparallel
 * latents) or a latent is zero: the linear form (1 - lam) za + lam zb.  lam = 0 returns za and lam = 1 returns zb bit for bit; masked
 * entries are exactly 0; nothing is re-centred (a linear combination of mean-free x parts is mean-free).  One launch per 64 frames,
 * stream-ordered, no host synchronisation; lam_host is read before the call returns.  HD_E_INVALID: L < 1, out overlapping za or zb. */
int hd_slerp(hd_handle* h, hd_topology* topo, const float* za, const float* zb, const float* lam_host, int L, float* out, void* stream);

/* ---- Classifier-free guidance (ABI 12, additive; no reference counterpart): every transition of a path loop evaluates the network
 * twice - under the context and under a second ("null") context - and the combination
 *     eps^ = eps_u + w (eps_c - eps_u)
 * goes into the unchanged update.  w sets how strongly a sample follows its context (w = 1: the conditional model, w = 0: the
 * unconditional one, w > 1: extrapolation).  Mechanism only: the model must have seen the null context in training (context dropout,
 * hierdiff_amd/guidance.py), and which w helps on a trained checkpoint is for the user to validate.  Nothing is drawn.
 *
 * hd_guide_combine: out[B,N,D] from eps_c, eps_u [B,N,D] and the DEVICE array w_dev of w_rows = 1 (shared) or B (per molecule) scales.
 * Per molecule: w_b == 1 copies eps_c and w_b == 0 copies eps_u bit for bit (rescale is ignored for these two values); otherwise
 * g = fmaf(w_b, eps_c - eps_u, eps_u) per entry and, with rescale = phi > 0, the noise-prediction form of "CFG rescale":
 *     out = f g,   f = fp32(phi sqrt(S_c / S_g) + (1 - phi)),
 * S_c / S_g the sums of squared deviations of eps_c / g from their means over the molecule's valid entries (node mask, all D columns),
 * accumulated in double in a fixed order (no atomics); S_g == 0 or a non-finite quotient gives f = 1.  phi == 0 runs no reduction.
 * Masked entries are exactly 0.  out may be eps_c itself.  Stream-ordered, no host synchronisation.  HD_E_INVALID: w_rows not 1 or B,
 * rescale outside [0, 1], out overlapping eps_u (or eps_c other than exactly).  The kernel stages nothing in LDS: any N * D. */
int hd_guide_combine(hd_handle* h, hd_topology* topo, const float* eps_c, const float* eps_u, const float* w_dev, int w_rows,
                     float rescale, float* out, void* stream);
/* hd_sample_path (fixed_mask == NULL) or hd_sample_path_inpaint (fixed_mask != NULL, its restrictions apply) with guidance: per
 * network call of the unguided loop two forwards at the same time value - context into the topology's eps, context_u into a second
 * topology-owned buffer, each with its own NaN guard - then hd_guide_combine in place, then the unchanged update.  Needs a path
 * (hd_set_path / hd_set_path_up), a context-conditioned model and both contexts [B,N,C]; whole molecules only (no pocket rows: there
 * is no mol_shape).  Draw layout: that of the unguided loop (hd_noise).  w_dev / w_rows / rescale as in hd_guide_combine.
 *   use_graph    ONE captured transition per topology in a graph of its own next to the unguided one (calls of either kind on one
 *                topology do not evict each other); context_u and w are replayed from library-owned copies like the context, so new
 *                values of w or of the contexts replay the cached graph.  Rebuilt when anything the unguided graph is keyed on
 *                changes, or w_rows, rescale or whether inpainting runs.  use_graph = 0 gives the same bits. */
int hd_sample_path_guided(hd_handle* h, hd_topology* topo, float* z, const float* context, const float* context_u, const float* w_dev,
                          int w_rows, float rescale, int k_lo, int k_hi, const float* raw_x, const float* raw_h, int noise_rows,
                          uint64_t seed, uint64_t sample_id_base, int use_graph, const uint8_t* fixed_mask, const float* xh_known,
                          int resamplings, void* stream);
/* Number of times the topology's captured guided transition was instantiated (-1: null topology). */
long long hd_guided_graph_builds(const hd_topology* topo);

/* ---- Second-order multistep sampling (ABI 12, additive; no reference counterpart): DPM-Solver++(2M) in data-prediction form on a
 * descending path.  With lambda = log(alpha / sigma) = -gamma / 2, h_k = lambda_s - lambda_t of transition k and r_k = h_{k-1} / h_k:
 *     x^_k = p z_t - q eps,        z_s = (a z_t - b eps) + c2 (x^_k - x^_{k-1}),
 *     a = alpha_s / alpha_t,  b = a sigma_t - sigma_s  (the eta = 0 row of hd_set_path),  p = 1 / alpha_t,  q = sigma_t / alpha_t,
 *     c2 = alpha_s (-expm1(-h_k)) / (2 r_k),
 * eps with its x part mean-removed and z_s re-centred as in the plain step.  A row with c2 == 0 reads no history and gives the bits
 * of the eta = 0 row {a, b, 0, 0}; nothing is drawn on the path.
 * hd_set_path_multistep: hd_set_path with host rows5 = K rows {a, b, c2, p, q} (form 2).  Validated like hd_set_path (descending,
 * chained, K <= T, schedule set); c2 of row 0 must be 0 (HD_E_INVALID).  hd_sample_path and hd_sample_path_guided (fixed_mask == NULL)
 * then run the path, with and without use_graph (one captured transition per topology, the row read through the device-side path
 * position); hd_sample_path_inpaint and guided calls with a fixed_mask are HD_E_INVALID.  Injected normals are not read.
 *   history   x^_{k-1} lives in a topology-owned buffer [B,N,D] (allocated by the first such call).  The topology remembers which
 *             path (every hd_set_path* call starts a new one) and which position k_hi its history belongs to: a call whose first row
 *             has c2 != 0 must have k_lo equal to that position on the same path, HD_E_STATE otherwise.  A call starting on a row
 *             with c2 == 0 (k_lo = 0) needs none. */
int hd_set_path_multistep(hd_handle* h, int K, const int* t_idx, const int* s_idx, const float* rows5);
/* The single update: x_out[B,N,D] = x^_k (masked entries 0) and zs[B,N,D] = z_s from zt, eps [B,N,D] (device) and the HOST row
 * row5 = {a, b, c2, p, q}.  x_prev [B,N,D] is x^_{k-1}; it may be NULL when c2 == 0 and is not read then.  zs may be zt and x_out may
 * be x_prev; any other overlap is HD_E_INVALID, as is N * D floats beyond one workgroup's LDS (64 KiB).  Stream-ordered. */
int hd_multistep_step(hd_handle* h, hd_topology* topo, const float* zt, const float* eps, const float* row5, const float* x_prev,
                      float* x_out, float* zs, void* stream);

/* ---- Stochastic second-order multistep sampling (ABI 12, additive; no reference counterpart): SDE-DPM-Solver++(2M), the multistep
 * correction on the ancestral update.  With h_k and r_k as above and xi a standard normal (x part mean-removed, masked):
 *     published   z_s = (sigma_s / sigma_t) e^{-h} z_t + alpha_s (1 - e^{-2h}) x^_k + 1/2 alpha_s (1 - e^{-2h}) (x^_k - x^_{k-1}) / r_k
 *                       + sigma_s sqrt(1 - e^{-2h}) xi,         x^_k = (z_t - sigma_t eps) / alpha_t
 *     as run      x^_k = p z_t - q eps,        z_s = ((a z_t - b eps) + c xi) + c2 (x^_k - x^_{k-1}),
 *     {a, b, c} = the eta = 1 linear row of hd_set_path (form 1): sigma_s sqrt(1 - e^{-2h}) is the ancestral sigma~,
 *     p = 1 / alpha_t,  q = sigma_t / alpha_t,  c2 = alpha_s (-expm1(-2 h_k)) / (2 r_k)       (-2 h where the 2M rows have -h),
 * eps and xi with their x parts mean-removed, z_s re-centred, rows >= mol_shape left alone, as in the plain step.  First order of
 * this family is ancestral sampling: a row with c2 == 0 reads no history and gives the bits of the form-1 row {a, b, c, 0} with
 * the same draws.  Which form is which: 0 ancestral rows, 1 linear rows (eta), 2 multistep rows5 (deterministic), 3 these rows6.
 * hd_set_path_multistep_sde: hd_set_path with host rows6 = K rows {a, b, c, c2, p, q} (form 3), validated like
 * hd_set_path_multistep; c2 of row 0 must be 0 (HD_E_INVALID).  hd_sample_path and hd_sample_path_guided (fixed_mask == NULL) then run
 * the path with and without use_graph; the draws (T - s of the arrival step) and injected normals (one pair per transition) are
 * those of form 1; the history buffer, its bookkeeping and the HD_E_STATE continuity rule are those of form 2.
 * hd_sample_path_inpaint and guided calls with a fixed_mask are HD_E_INVALID (a jump back invalidates the history).
 * Steering (hd_steer_attach) is allowed - the update draws - and the history follows its lineage: rows that receive another
 * row's z_t and eps^ receive its x^_{k-1} too, inside the captured transition. */
int hd_set_path_multistep_sde(hd_handle* h, int K, const int* t_idx, const int* s_idx, const float* rows6);
/* The single update: x_out[B,N,D] = x^_k (masked entries 0) and zs[B,N,D] = z_s from zt, eps [B,N,D] (device) and the HOST row
 * row6 = {a, b, c, c2, p, q}.  x_prev as in hd_multistep_step (NULL allowed when c2 == 0).  Noise: raw_x [rows][mol][3] and raw_h
 * [rows][mol][F] (device; noise_rows = 1 shares one row), or both NULL for the counter-based generator at (seed, sample_id_base + b
 * - or sample_id_base for every row when share_rows != 0 -, draw).  mol_shape: rows >= mol_shape of a molecule are left alone (< 0
 * or > N: N).  zs may be zt and x_out may be x_prev; any other overlap is HD_E_INVALID, as is mol * D floats beyond one workgroup's
 * LDS (64 KiB).  Stream-ordered. */
int hd_multistep_sde_step(hd_handle* h, hd_topology* topo, const float* zt, const float* eps, const float* row6, const float* x_prev,
                          float* x_out, const float* raw_x, const float* raw_h, int noise_rows, uint64_t seed,
                          uint64_t sample_id_base, uint32_t draw, int share_rows, int mol_shape, float* zs, void* stream);

/* ---- Recording a trajectory (ABI 12, additive; the reference's sample_chain, en_diffusion.py:669-710): the path loops write
 * intermediate states into a caller-owned sink chain[frames][B][N][D] (device, fp32) while they run - one more element-wise launch
 * per transition (k_chain_frame), inside the captured transition when use_graph is set.  Frames are in data units, `unnormalize`
 * applied as a multiply and then an add (never fused):  x = v nv0,  h = (v nv1 + nb1) mask,  padded rows exactly 0.
 * hd_set_chain: the tables of the CURRENT path (hd_set_path*; every new path needs its own call, HD_E_STATE from the loops
 * otherwise): frame_of[K], the frame transition k writes or -1 for none, and - needed for what = 1 only, else NULL -
 * alpha_sigma[K][2] = {alpha_t, sigma_t} of every transition's departure level.  HD_E_INVALID: K != the path's K, an entry outside
 * [-1, frames).  HD_E_STATE: no path set for the current schedule.
 * hd_chain_attach: from now on every path-loop entry point on this topology (hd_sample_path, hd_sample_path_inpaint,
 * hd_sample_path_guided; every row form, ascending paths included; with and without use_graph) records into `chain`, whose
 * `frames` must equal hd_set_chain's:
 *   what = 0   the state behind transition k (behind the last round's replacement when inpainting),
 *   what = 1   the data prediction x^ = 1 / alpha_t (z_t - sigma_t eps^) of transition k (of its last round), eps^ the - guided -
 *              network output, taken between the network call and the update.
 * Whole molecules only (mol_shape < N is HD_E_INVALID while a sink is attached).  Recording changes no sample: z is only read.
 * hd_chain_detach: stop recording; the unrecorded launches, graphs, keys and build counters are exactly those of a topology
 * that never recorded.  hd_sample_loop and hd_sample_loop_inpaint never record: they run the path loop on the handle's every-step
 * tables, and the chain tables and the sink belong to the caller's path (to record a full chain, upload the identity path).
 *   use_graph    the recording transition is ONE more graph per topology next to the plain and the guided one (none evicts another).
 *                The sink's address is not baked in: it lives in a device word the loop's state kernel sets, so a new sink
 *                replays the cached graph.  Rebuilt when anything the unrecorded graph is keyed on changes, or what, nv0, nv1, nb1,
 *                or the tables (every hd_set_chain). */
int hd_set_chain(hd_handle* h, int K, const int* frame_of, const float* alpha_sigma, int frames);
int hd_chain_attach(hd_topology* topo, float* chain, int frames, int what, float nv0, float nv1, float nb1);
int hd_chain_detach(hd_topology* topo);
/* Number of times the topology's captured recording transition was instantiated (-1: null topology). */
long long hd_chain_graph_builds(const hd_topology* topo);

/* ---- Restraint-guided sampling (ABI 12, additive; no reference counterpart): at every transition of a path loop an energy U is
 * evaluated on the network's data prediction and its gradient is added into the noise prediction; the update that follows -
 * ancestral, eta < 1, multistep - and a record = "x0" frame read the changed eps^.  One more launch per transition (k_restrain_eps),
 * between the (guided) network call and everything that reads eps^, inside the captured transition when use_graph is set.
 * FRAME: coordinates are x = nv0 z_x in the model's frame, which has the centre of mass of the molecule's valid nodes at the
 * origin.  Obstacles and anchors are given in that frame: the caller places them relative to where the molecule's centre sits.
 * Tables, per molecule (every table has 1 row, shared by all molecules, or B rows; device or host pointers, fp32 / int32):
 *   obs      [rows][P][5] = (y_x, y_y, y_z, r, k)     U_obs  = 1/2 sum_{i valid} sum_p k_p max(0, r_p - |x_i - y_p|)^2
 *                                                     a row with r <= 0 or k <= 0 is padding
 *   pair_idx [rows][Q][2], pair_f [rows][Q][3] = (lo, hi, k)
 *                                                     U_pair = 1/2 sum_q k_q (max(0, d - hi)^2 + max(0, lo - d)^2), d = |x_i - x_j|
 *   anc_idx  [rows][A],    anc_f [rows][A][5] = (a_x, a_y, a_z, r, k)
 *                                                     U_anc  = 1/2 sum_a k_a max(0, |x_i - a| - r)^2
 * A pair / anchor row whose node index is negative (-1: padding), >= N or masked in that molecule is inactive - not an error, sizes
 * are drawn.  A term at distance exactly 0 contributes no gradient.
 * The update of transition k with the row {alpha_t, sigma_t, lambda_k, clip_k} and the scale s_b of molecule b:
 *   x^0_i   = nv0 (1 / alpha_t) (z_x,i - sigma_t eps_x,i)        fp32, the operations and the order of a record = "x0" frame
 *   Delta_i = s_b lambda_k dU/dx_i (x^0), valid nodes            double; |Delta_i| > clip_k: scaled to length clip_k (inf: no clip)
 *   Delta_i -= mean over the valid nodes of Delta                eps_x stays free of centre of mass
 *   eps_x,i += Delta_i                                           one rounding to fp32; feature columns and masked rows untouched
 * s_b lambda_k == 0: the molecule's workgroup writes nothing, and an entry whose Delta is exactly 0 keeps its bits.  Every sum has a
 * fixed order that depends on (N, P, Q, A) alone: a sample depends on its id, mask, weights, schedule, path and its own rows only.
 * hd_set_restraint: the rows4[K][4] (host) of the CURRENT path (hd_set_path*; every new path needs its own call, HD_E_STATE from
 *   the loops otherwise).  HD_E_INVALID: K != the path's K, alpha_t <= 0, sigma_t < 0, a non-finite lambda_k, clip_k <= 0.
 * hd_restraint_attach: copies the tables and scale[scale_rows] (stream-ordered) into buffers the topology owns; from now on
 *   hd_sample_path and hd_sample_path_guided (fixed_mask == NULL) on this topology are restrained; hd_sample_path_inpaint and
 *   guided calls with a fixed_mask are HD_E_INVALID while attached (inpainting re-centres on the known fragments: its frame
 *   moves; hd_restraint_frame below is the way to restrain them), as is mol_shape < N.  hd_sample_loop* ignore attached restraints, as they ignore chain sinks.
 *   HD_E_INVALID: a row count other than 1 or B, negative P / Q / A, nv0 not positive, N * 3 floats beyond one workgroup's LDS.
 * hd_restraint_detach: the launches, graphs and keys are again exactly those of a topology that never had restraints.
 *   use_graph    the restrained transition lives in the slot of its unrestrained kind (plain, guided, recording) under a key that
 *                tells the two apart: a restrained call followed by an unrestrained one rebuilds and gives the unrestrained bits.
 *                Re-attaching tables of the same sizes, new scales, and hd_set_restraint with the same K are copies: the cached
 *                graph replays (hd_path_graph_builds / hd_guided_graph_builds / hd_chain_graph_builds do not move).  A table that
 *                outgrows its buffer, another row count or nv0 rebuild it once.
 * hd_restrain_eps: the single update above on given tensors with a host row4; out may be eps itself, nothing else may overlap.
 * hd_restraint_energy: out3[B][3] = (U_obs, U_pair, U_anc) in double for positions x[B][N][3] (fp32, data units) under the
 *   attached tables and the topology's mask.  Both are stream-ordered and need attached restraints (HD_E_STATE otherwise).
 * THE KNOWN FRAGMENTS' FRAME (additive): hd_restraint_frame(topo, 1) reads the attached tables in the coordinates of the xh_known of
 *   an inpainting call, the one mode whose known rows come back as a pure translation of the input.  With F the valid fixed nodes
 *   of a molecule and xk = nv0 xh_known_x (as uploaded, not centred):
 *     tau     = mean_F(x^0) - mean_F(xk)                         double; no fixed node: tau = 0 and every node is free (the plain update)
 *     U       = the three energies with the obstacle and anchor centres at y + tau; pairs do not see tau
 *     Delta_i = clip(s_b lambda_k dU/dx_i), tau held constant    free valid nodes only; a fixed node's Delta is 0 (the block is the
 *                                                                frame, its own clashes are the caller's input); a pair between a free
 *                                                                and a fixed node acts on the free one
 *     eps_x,i += Delta_i - mean over ALL valid nodes of Delta    fixed nodes receive -mean: eps_x stays mean-free, and behind the
 *                                                                posterior step and the replacement a free node has moved relative
 *                                                                to the block by its own Delta_i times the step's coefficient
 *   Frame 0 is the model's frame; hd_restraint_attach resets to it.  HD_E_STATE: no restraints attached.  While frame 1 is set,
 *   hd_sample_path_inpaint and guided calls with a fixed_mask run the framed update (k_restrain_eps<true>) in every resampling round,
 *   behind guidance; calls without fixed fragments and topologies with steering attached are HD_E_INVALID.  The frame is part of the
 *   graph key: switching it rebuilds the captured transition once, re-attaching tables of the same sizes does not.
 * hd_restrain_eps_framed: the single framed update on given tensors (fixed_mask u8 [B*N], xh_known [B][N][D] normalised); the
 *   aliasing rules of hd_restrain_eps, and out may not overlap xh_known.  Independent of hd_restraint_frame.
 * hd_restraint_energy_framed: out3 as hd_restraint_energy with tau = mean_F(x) - mean_F(x_known) of the given data-unit
 *   x / x_known [B][N][3]; shift3 [B][3] double receives tau (NULL: not wanted). */
int hd_set_restraint(hd_handle* h, int K, const float* rows4);
int hd_restraint_attach(hd_topology* topo, const float* obs, int obs_rows, int P, const int* pair_idx, const float* pair_f,
                        int pair_rows, int Q, const int* anc_idx, const float* anc_f, int anc_rows, int A, const float* scale,
                        int scale_rows, float nv0, void* stream);
int hd_restraint_detach(hd_topology* topo);
int hd_restrain_eps(hd_handle* h, hd_topology* topo, const float* z, const float* eps, const float* row4, float* out, void* stream);
int hd_restraint_energy(hd_handle* h, hd_topology* topo, const float* x, double* out3, void* stream);
int hd_restraint_frame(hd_topology* topo, int frame);
int hd_restrain_eps_framed(hd_handle* h, hd_topology* topo, const float* z, const float* eps, const float* row4,
                           const uint8_t* fixed_mask, const float* xh_known, float* out, void* stream);
int hd_restraint_energy_framed(hd_handle* h, hd_topology* topo, const float* x, const uint8_t* fixed_mask, const float* x_known,
                               double* out3, double* shift3, void* stream);

/* ---- Field restraints (ABI 12, additive; no reference counterpart): scalar potentials on regular 3-D lattices as a fourth term of
 * the restraint energy, read by trilinear interpolation - 8 loads per node and field, whatever the potential was rasterised from.
 * A topology with attached restraints carries up to HD_MAX_FIELDS fields.  Field f:
 *   values   v_f [n0][n1][n2] fp32, the last axis fastest, every n_c >= 2, n0 n1 n2 < 2^31; the pool `values` holds field f at
 *            offsets[f] .. offsets[f + 1] (offsets[0] = 0; device or host pointer)
 *   dims     [NF][3] = (n0, n1, n2)                                  host
 *   geom     [NF][8] = (o_x, o_y, o_z, h_x, h_y, h_z, k, wall)       host; origin, spacing > 0 per axis, stiffness k >= 0, wall >= 0
 *   weights  [w_rows][NF][N] fp32 >= 0, w_rows = 1 (shared) or B     device or host pointer
 * For a valid node i at x (the fp32 x^0 of the restraint update, or the given x of the energy calls), per axis c, in double:
 *   p_c   = x_c - tau_c                              tau = 0 in the model's frame; the known fragments' tau in frame 1
 *   u_c   = (p_c - o_c) / h_c,  ub_c = min(max(u_c, 0), n_c - 1),  cell_c = min((int)floor(ub_c), n_c - 2),  t_c = ub_c - cell_c
 *   V     = sum_{a,b,c in {0,1}} v[cell_0 + a][cell_1 + b][cell_2 + c] W_a(t_0) W_b(t_1) W_c(t_2),  W_0(t) = 1 - t, W_1(t) = t
 *   out_c = (u_c - ub_c) h_c                         how far outside the box, data units
 *   E     = k w_i (V + 1/2 wall sum_c out_c^2)
 *   dE/dx_c = k w_i ([0 <= u_c <= n_c - 1] (1 / h_c) dV/dt_c + wall out_c)
 *   U_fld = sum_f sum_{i valid} E                    may be negative: the values may be
 * On an interior lattice plane the gradient is the right-hand cell's; at u_c = n_c - 1 it is the last cell's with t = 1.  Outside the
 * box an axis contributes only the wall.  A node with a non-finite coordinate contributes neither energy nor gradient.  A term with
 * k w_i = 0 is skipped.  The gradient joins dU/dx_i of the update above, ahead of the clip and the mean; in frame 1 it sees tau, only
 * free nodes gather it, and the energy sums over all valid nodes.  hd_steer_step and the steered loops weigh on
 * ((U_obs + U_pair) + U_anc) + U_fld.  No atomics; every sum has a fixed order that depends on (N, NF) alone.
 * hd_restraint_fields: stream-ordered copies into buffers the topology owns (grown as the tables of hd_restraint_attach are).  Needs
 *   attached restraints (HD_E_STATE).  hd_restraint_attach resets the topology to NO fields, as it resets the frame: the order is
 *   attach -> fields -> frame.  NF = 0 clears the fields.  HD_E_INVALID: NF outside 0 .. 8, a dim < 2, a lattice of 2^31 values or
 *   more, a non-finite or non-positive spacing, a non-finite origin, a negative or non-finite k / wall, offsets that are not the
 *   running sums of n0 n1 n2, w_rows other than 1 or B, a null pointer with NF > 0.
 *   use_graph    re-attaching fields of the same sizes is a copy: the cached transition replays.  Another NF, a pool or weights that
 *                outgrow their buffer, or another w_rows rebuild once; a fielded call followed by an unfielded one on the same
 *                topology rebuilds and gives the bits of a topology that never had fields.
 * hd_restraint_field_energy: out[B] = U_fld in double for positions x[B][N][3] (fp32, data units) under the topology's mask.
 * hd_restraint_field_energy_framed: the same with tau = mean_F(x) - mean_F(x_known); shift3 [B][3] double receives tau (NULL: not
 *   wanted).  Both are stream-ordered and need attached restraints (HD_E_STATE otherwise); without fields they write 0. */
#define HD_MAX_FIELDS 8
int hd_restraint_fields(hd_topology* topo, int NF, const float* values, const long long* offsets, const int* dims, const float* geom,
                        const float* weights, int w_rows, void* stream);
int hd_restraint_field_energy(hd_handle* h, hd_topology* topo, const float* x, double* out, void* stream);
int hd_restraint_field_energy_framed(hd_handle* h, hd_topology* topo, const float* x, const uint8_t* fixed_mask, const float* x_known,
                                     double* out, double* shift3, void* stream);

/* ---- Template restraints (ABI 12, additive; no reference counterpart): the optimal rigid superposition (Kabsch) of the data
 * prediction onto a 3-D template as a fifth term of the restraint energy - "lay these nodes out like this arrangement, wherever and
 * however the molecule ends up oriented".  A topology with attached restraints carries up to HD_MAX_TEMPLATES templates of M rows:
 *   idx   [rows][NT][M] int32          the node i_m a row names; rows = 1 (shared) or B          host
 *   f     [rows][NT][M][4] fp32        (y_x, y_y, y_z, w): the template position and the weight  host
 *   geom  [NT][2] fp32                 (k >= 0, fit: 0 rigid, 1 translation only)                host
 * A row is ACTIVE in molecule b when 0 <= i_m < N, node i_m is valid in b and w_m > 0 (a row that names a node the molecule lacks is
 * inactive, as for anchors; pad a short template with w = 0).  Over the active rows, in double, on the fp32 x^0 of the restraint
 * update or the given x of the energy call:
 *   W = sum w_m,  c_x = sum w_m x_{i_m} / W,  c_y = sum w_m y_m / W,  x'_m = x_{i_m} - c_x,  y'_m = y_m - c_y
 *   S = sum w_m x'_m y'_m^T,  R = argmax_{R in SO(3)} tr(R^T S)  (fit 1: R = I)      a proper rotation: a mirror image does not fit
 *   r_m = x'_m - R y'_m,  U_tpl,t = 1/2 k_t sum w_m |r_m|^2,  rmsd_t = sqrt(sum w_m |r_m|^2 / W)
 *   dU_tpl,t/dx_{i_m} += k_t w_m r_m        exact: R maximises, so its dependence on x drops out, and sum w_m r_m = 0
 * R comes from Horn's quaternion form, the eigenvector of the largest eigenvalue of a symmetric 4x4 matrix by a cyclic Jacobi
 * iteration of a fixed number of sweeps: deterministic, and independent of the molecule's place in the batch.  R is unique iff
 * sigma_2 + sign(det S) sigma_3 > 0 for the singular values of S; otherwise (two active rows, collinear rows) some maximiser is used -
 * the energy is unique, the gradient finite.  W = 0, exactly one active row, or a non-finite active coordinate: the template
 * contributes neither energy nor gradient to that molecule.  The gradient joins dU/dx_i of the update above behind the fields, ahead
 * of the scale, the clip and the mean.  A template does not see tau: it carries its own frame.  In frame 1 rows on fixed nodes take
 * part in the fit and the energy, only free nodes gather a gradient, and fixed nodes receive -mean like every valid node.
 * hd_steer_step and the steered loops weigh on (((U_obs + U_pair) + U_anc) + U_fld) + U_tpl, U_tpl = ((U_0 + U_1) + U_2) + U_3.
 * No atomics; every sum has a fixed order that depends on (N, M) alone.
 * hd_restraint_templates: stream-ordered copies into buffers the topology owns.  Needs attached restraints (HD_E_STATE).
 *   hd_restraint_attach resets the topology to NO templates, as it resets the fields and the frame; the order of the fields and the
 *   templates calls is free.  NT = 0 clears the templates.  HD_E_INVALID: NT outside 0 .. 4, M < 1, rows other than 1 or B, a negative
 *   or non-finite k or w, a non-finite y, a fit other than 0 or 1, a null pointer with NT > 0.
 *   use_graph    re-attaching tables of the same (NT, M, rows) is a copy: the cached transition replays.  Other sizes rebuild once; a
 *                templated call followed by an untemplated one on the same topology rebuilds and gives the bits of a topology that
 *                never had templates.
 * hd_restraint_template_energy: out [B][NT] = U_tpl,t in double for positions x [B][N][3] (fp32, data units) under the topology's mask;
 *   fit16 [B][NT][16] (NULL: not wanted) = (R row-major [9], c_x [3], c_y [3], rmsd): x_{template frame} = R^T (x - c_x) + c_y.  A
 *   template that contributes nothing to a molecule reports U = 0, R = I, c_x = c_y = 0, rmsd = 0.  Stream-ordered.  Without attached
 *   restraints or without templates it writes nothing and returns HD_E_STATE. */
#define HD_MAX_TEMPLATES 4
int hd_restraint_templates(hd_topology* topo, int NT, int rows, int M, const int* idx, const float* f, const float* geom, void* stream);
int hd_restraint_template_energy(hd_handle* h, hd_topology* topo, const float* x, double* out, double* fit16, void* stream);

/* ---- Feature restraints (additive, ABI number unchanged; no reference counterpart): bands and molecule-wide sums on the features h
 * of the data prediction, k_restrain_feat.hpp.  For a valid node i and channel c in [0, F), F = D - 3, in data units, with the fp32
 * operations and the order of a record="x0" frame:
 *   v_ic = fadd(fmul(fmul(1 / alpha_t, fsub(z[i,3+c], fmul(sigma_t, eps^[i,3+c]))), nv1), nb1)
 * eps^ behind guidance and the position update (which does not touch the feature columns).  Everything below in double.
 *   bands   lo, hi, k [band_rows][W][F], W <= N (nodes i >= W have none).  Element (i, c) is active when node i is valid, k_ic > 0 and
 *           v_ic is finite:  U_band = 1/2 sum k_ic (max(0, v - hi)^2 + max(0, lo - v)^2),  dU/dv_ic = k_ic (max(0, v - hi) - max(0, lo - v)).
 *           lo = -inf / hi = +inf: one-sided; lo = hi: a harmonic target; v on a bound: energy 0, gradient 0.
 *   sums    at most HD_MAX_FEATURE_SUMS rows: coef [sum_rows][S][F], sum_f [sum_rows][S][4] = (lo, hi, k, reduce: 0 sum, 1 mean).
 *           s_r = sum_{i valid} sum_c coef_rc v_ic,  n = valid nodes,  m_r = s_r or s_r / n,
 *           U_sum = 1/2 sum_r k_r (max(0, m_r - hi_r)^2 + max(0, lo_r - m_r)^2),  dU/dv_ic += k_r (...) coef_rc (1 or 1 / n).
 *           A row is inactive when k_r <= 0 or n = 0; it contributes nothing when a valid v it reads with a non-zero coefficient is
 *           not finite.
 *   update  eps^[i,3+c] += clip_i(s_b lambda_k ratio dU_feat/dv_ic) for valid nodes, U_feat = U_band + U_sum: s_b the molecule's scale
 *           (hd_restraint_attach), lambda_k and clip_k the handle's restraint rows (hd_set_restraint), the clip on the Euclidean norm
 *           over the node's F steps (apart from the position step's); no mean is removed.  An element whose step is exactly 0 keeps its
 *           bits; position columns and masked rows are never written; s_b lambda_k ratio = 0 writes nothing.
 * hd_restraint_features: HOST arrays, copied into library-owned buffers; call it behind hd_restraint_attach, which resets to "no
 *   features" (in any order with hd_restraint_fields / _templates).  rows = 1 (shared) or B.  W = 0: no bands, S = 0: no sums, both 0:
 *   no features.  ratio: 1, or nv1 / nv0 when lambda_k is the score weight nv0 sigma_t / alpha_t (dv / dz_h = nv1 / alpha_t).
 *   HD_E_INVALID: null pointers, S > 8, W > N, rows not in {1, B}, non-finite k / coef / nv1 / nb1 / ratio, lo > hi, NaN bounds, reduce
 *   not in {0, 1}; HD_E_STATE: no restraints attached.  A path loop then launches k_restrain_feat behind the position update in every
 *   transition (in the known fragments' frame too: features have no frame, it acts on all valid nodes and the replacement step
 *   overwrites known elements afterwards), and steering weighs on ((((U_obs + U_pair) + U_anc) + U_fld) + U_tpl) + U_feat.
 *   use_graph    re-attaching tables of the same (W, S, rows, nv1, nb1, ratio) is a copy: the cached transition replays.  Anything else
 *                rebuilds once; a featured call followed by an unfeatured one rebuilds once and gives the bits of a topology that never
 *                had features.
 * hd_restrain_feat: the single update on (z, eps) with the row {alpha_t, sigma_t, lambda, clip}, out of place or in place (out == eps).
 * hd_restraint_feature_energy: out2 [B][2] = (U_band, U_sum) in double for features h [B][N][F] (fp32, data units) under the
 *   topology's mask; sums [B][S] (NULL: not wanted) = m_r, 0 for a row that is inactive or contributes nothing.  Stream-ordered.
 *   Both return HD_E_STATE without attached restraints or features and then write nothing. */
#define HD_MAX_FEATURE_SUMS 8
int hd_restraint_features(hd_topology* topo, const float* lo, const float* hi, const float* k, int band_rows, int W, const float* coef,
                          const float* sum_f, int sum_rows, int S, float nv1, float nb1, float ratio, void* stream);
int hd_restrain_feat(hd_handle* h, hd_topology* topo, const float* z, const float* eps, const float* row4, float* out, void* stream);
int hd_restraint_feature_energy(hd_handle* h, hd_topology* topo, const float* hf, double* out2, double* sums, void* stream);

/* ---- Steered sampling (ABI 12, additive; no reference counterpart): sequential Monte-Carlo steering of a restrained path loop.
 * The batch is G groups of P rows (particles); group g owns rows g P .. g P + P - 1, which the CALLER guarantees to have equal
 * masks, contexts and restraint rows.  At every transition k, behind the network call, guidance and the restraint update of eps^:
 *   U(b)     = U_obs + U_pair + U_anc of row b's data prediction x^0 (the fp32 x^0 of the restraint update; the energy in double)
 *   logw[b] += -beta_k (U(b) - U_prev[b]);  U_prev[b] = U(b)       a non-finite U or update: logw[b] = -inf (weight 0)
 *   per group: w_i = exp(logw_i - max), S = sum w, ESS = S^2 / sum w^2 (sums in index order).  ESS < ess P: systematic resampling
 *     with one uniform u - anc[j] = the smallest i whose inclusive prefix sum of w exceeds (u + j) / P * S - and rows with
 *     anc[j] != j receive z_t, eps^, U_prev and the lineage root of row anc[j]; the group's logw is reset to 0.  Otherwise, and in a
 *     group whose weights are all 0 (counted), nothing moves.
 * The posterior step follows with every row's own noise, so duplicates diverge: steering needs noise_rows == B and a stochastic
 * update (the deterministic multistep rows of form 2 are HD_E_INVALID; the stochastic ones of form 3 are allowed, and their history
 * x^_{k-1} moves with z_t and eps^).  u = hd_philox_uniform_host(seed, sample_id_base + g P, the transition's draw T - s,
 * 0xfffffffe).  Four more launches per transition (k_steer_weigh, k_steer_resample, two of k_steer_gather), plain kernel nodes of
 * a captured transition.  A group's result depends on the seed, the ids of its rows, P, its masks and tables, the weights, the
 * schedule and the path only - not on other groups, graph replay or how the chain is cut into calls.
 * hd_set_steer: the rows3[K][3] = {alpha_t, sigma_t, beta_k} (host) of the CURRENT path, as hd_set_restraint.  HD_E_INVALID: K != the
 *   path's K, alpha_t <= 0, sigma_t < 0, beta_k negative or non-finite.
 * hd_steer_attach: from now on hd_sample_path / hd_sample_path_guided on this topology are steered; they need attached restraints
 *   (hd_restraint_attach; a scale of 0 steers without the gradient update) and the rows of hd_set_steer.  The steering state
 *   (logw, U_prev, roots, statistics) belongs to the topology and survives between calls: reset != 0 starts a chain (logw = U_prev =
 *   0, root[b] = b mod P), reset == 0 continues the one the last call left (HD_E_STATE when there is none for this P).
 *   HD_E_INVALID: P outside 2 .. 256, B not a multiple of P, ess outside (0, 1].  Re-attaching with the same P and ess replays
 *   the cached graph.
 * hd_steer_detach: the launches, graphs and keys are again those of a topology that never was steered.
 * hd_steer_step: the stage above once, on given tensors z, eps [B][N][D] (both rewritten in the moved rows) with a host row3.
 * hd_steer_read: stream-ordered copies of the state into host or device buffers, any of which may be NULL: logw [B], uprev [B]
 *   (double), root [B], anc [B] (int32; anc: the source ROW of the latest transition), stats [B / P][3] (double: resampling events,
 *   the smallest ESS, transitions in which every weight was 0) since the last reset. */
int hd_set_steer(hd_handle* h, int K, const float* rows3);
int hd_steer_attach(hd_topology* topo, int P, double ess, int reset, void* stream);
int hd_steer_detach(hd_topology* topo);
int hd_steer_step(hd_handle* h, hd_topology* topo, float* z, float* eps, const float* row3, uint32_t draw, uint64_t seed,
                  uint64_t sample_id_base, void* stream);
int hd_steer_read(hd_topology* topo, double* logw, double* uprev, int* root, int* anc, double* stats, void* stream);

/* ---- Diverse sampling (ABI 12, additive; no reference counterpart): the rows of a group repel each other by their aligned RMSD
 * (particle guidance).  The batch is G groups of P rows; group g owns rows g P .. g P + P - 1 (the layout of steering), and groups
 * never interact.  At every transition k, behind the network call, guidance and the restraint updates of eps^, per group, in double on
 * the fp32 data predictions x^0 of its rows (those of the restraint update, nv0 included):
 *   pair p < q:  A = the nodes valid in both rows, n = |A|;  c_p, c_q = the centroids over A;  S = sum_A (x_p - c_p)(x_q - c_q)^T;
 *                R = argmax_{R in SO(3)} tr(R^T S) (a proper rotation: mirror images stay apart);  r_i = (x_p,i - c_p) - R (x_q,i - c_q);
 *                d2 = sum_A |r_i|^2 / n;  e = exp(-d2 / (2 length^2))
 *   Phi = kappa sum_{p<q} e;   dPhi/dx_p,i = -(kappa / (length^2 n)) sum_{q != p} e r_i  (on the q side r_i = (x_q,i - c_q) - R^T (x_p,i - c_p));
 *   exact without dR/dx because R maximises and sum_A r = 0.  The partners q are added in ascending order.
 *   step_{p,i} = s_g lambda_k dPhi/dx_p,i, clipped per node to clip_k, the mean over the row's valid nodes removed;
 *   eps^_x[p,i] = fp32(double(eps^_x) + step) on valid nodes; an element whose step is exactly 0 keeps its bits; feature columns and
 *   masked rows are never written; s_g lambda_k == 0 writes nothing.
 * A pair with n <= 1, or with a non-finite coordinate on a node of A, contributes nothing to either side.  With n = 2 or collinear
 * nodes R is not unique; d2 is, and the gradient is finite.  One launch (k_diverse_eps), one workgroup per group, no atomics, nothing
 * is drawn; every sum runs in an order that depends on (N, P) alone.  A group's result depends on the seed, the ids of its rows, P, its
 * masks, contexts and tables, the weights, the schedule and the path only - not on other groups, graph replay or how the chain is cut
 * into calls.  No state crosses transitions.
 * hd_set_diversity: the rows4[K][4] = {alpha_t, sigma_t, lambda_k, clip_k} (host) of the CURRENT path, checked as hd_set_restraint's.
 * hd_diversity_attach: from now on hd_sample_path / hd_sample_path_guided on this topology carry the update, behind the restraint
 *   updates, ahead of a recorded data prediction.  scale: host [scale_rows] s_g, scale_rows = 1 (shared) or B / P; nv0 as in
 *   hd_restraint_attach.  HD_E_INVALID: P outside 2 .. 32, B not a multiple of P, kappa negative, length or nv0 not positive, anything
 *   non-finite, or P * N * 3 floats plus P (P - 1) / 2 pair records of 96 bytes beyond one workgroup's LDS (64 KB).  Re-attaching with
 *   the same sizes and numbers replays the cached graph; another P, scale_rows, kappa, length or nv0 rebuilds it once.
 *   The path loop then refuses, behind every older refusal: an inpainting call, mol_shape < N, steering attached at the same time
 *   (HD_E_INVALID), rows not set for the current path (HD_E_STATE), noise_rows == 1 on a range with a row that draws (HD_E_INVALID).
 * hd_diversity_detach: the launches, graphs and keys are again those of a topology that never had it.
 * hd_diverse_eps: the update once on given tensors with a host row4; the aliasing rules of hd_restrain_eps.
 * hd_diversity_energy: for positions x [B][N][3] in data units Phi per group into phi [G] and, unless NULL, the aligned RMSD matrix
 *   into rmsd [G][P][P] (device doubles): symmetric, zero diagonal, NaN for a pair that contributes nothing. */
int hd_set_diversity(hd_handle* h, int K, const float* rows4);
int hd_diversity_attach(hd_topology* topo, int P, double kappa, double length, const float* scale, int scale_rows, float nv0, void* stream);
int hd_diversity_detach(hd_topology* topo);
int hd_diverse_eps(hd_handle* h, hd_topology* topo, const float* z, const float* eps, const float* row4, float* out, void* stream);
int hd_diversity_energy(hd_handle* h, hd_topology* topo, const float* x, double* phi, double* rmsd, void* stream);

/* ---- Predictor-corrector sampling (ABI 12, additive; no reference counterpart): Langevin correctors in the path loop (Song et al.
 * 2021; Du et al. 2023).  A corrector acts at the DEPARTURE level t_k of transition k, ahead of that transition's predictor call: it
 * reads the same network-time word and row k of every term's table as the predictor does.  Level 0 never gets one (the decode follows
 * it); level T (or t_start) does.  Transition k becomes
 *     C times:  the network call with the launches the predictor's call gets (guidance, restraints, feature restraints, diversity),
 *               then one Langevin step on z at level t_k (k_langevin_step);
 *     then:     the predictor's own network call (+ the same terms, + a recorded data prediction) and the unchanged posterior step.
 * The Langevin step, per molecule b on row k = {sigma_t, q_k, g_max_k}:
 *     eps~ = eps^ with its x part freed of the mean over the valid nodes;  xi~ = normals, masked, the x part freed of its mean (both
 *     as the posterior step forms them; the two means are double sums, rounded once);  n_xi^2 = sum xi~^2,  n_eps^2 = sum eps~^2
 *     over the valid nodes and all D columns, of the deviations from the double means, summed in double in an order that depends on
 *     (N, D) alone;
 *     g_b = q_k (mode "fixed", adaptive = 0)   or   g_b = min(g_max_k, q_k n_xi^2 / n_eps^2) (mode "snr", adaptive = 1);
 *     z' = (z - (g_b sigma_t) eps~) + (sigma_t sqrt(2 g_b)) xi~: both coefficients formed in double and rounded once to fp32, the
 *     expression in fp32 in this order, the x part re-centred over the valid nodes
 * - that is z + delta score + sqrt(2 delta) xi with score = -eps^ / sigma_t and delta = g_b sigma_t^2.  Masked rows are never written.
 * A molecule keeps its bits (gain 0) when g_b == 0, when n_eps^2 is not greater than 0, when a norm or the gain is not finite, or when
 * it has no valid node.  A row with q_k == 0 draws nothing and writes nothing.
 * Noise: corrector step c of transition k draws on stream 1 + c of the loop's layout, draw = (T + 2) (1 + c) + (T - s_k), element
 * index and sample id as in the posterior step: the predictor's draws do not move, a sample depends on its global id, mask, weights,
 * schedule, path and C only, and chains cut into calls give the bits of the whole.  noise_rows == 1 shares one row.  Multistep rows
 * keep their history: only the predictor reads and writes it.
 * hd_set_corrector: rows3[K][3] = {sigma_t, q_k, g_max_k} (host) of the CURRENT path.  HD_E_INVALID unless sigma_t >= 0, q_k >= 0 and
 *   finite, g_max_k > 0 (inf: no cap).
 * hd_corrector_attach: from now on hd_sample_path / hd_sample_path_guided on this topology run C (1 .. HD_MAX_CORRECTORS) corrector
 *   steps per transition.  Re-attaching the same C and mode with rows of the same size replays the cached graph; another C or mode
 *   rebuilds it once.  The path loop then refuses, behind every older refusal: an inpainting call, steering attached at the same time,
 *   mol_shape < N, injected noise - its K + 2 rows hold none for correctors - (HD_E_INVALID); rows not set for the current path
 *   (HD_E_STATE).
 * hd_corrector_detach: the launches, graphs and keys are again those of a topology that never had it.
 * hd_corrector_read: the gains g_b of the last transition that ran into gains [C][B] doubles (host or device), stream-ordered.
 * hd_langevin_step: the step once on given tensors with a host row3.  out may be z itself (in place), not a shifted overlap of it,
 *   and may not overlap eps.  raw_x / raw_h [noise_rows][N][3] / [N][F]: injected normals, or both NULL for the generator at (seed,
 *   sample_id_base + b, draw); noise_rows 1 (one shared row) or B.  gain_out: device [B] doubles or NULL. */
#define HD_MAX_CORRECTORS 8
int hd_set_corrector(hd_handle* h, int K, const float* rows3);
int hd_corrector_attach(hd_topology* topo, int C, int adaptive, void* stream);
int hd_corrector_detach(hd_topology* topo);
int hd_corrector_read(hd_topology* topo, double* gains, void* stream);
int hd_langevin_step(hd_handle* h, hd_topology* topo, const float* z, const float* eps, const float* row3, int adaptive,
                     const float* raw_x, const float* raw_h, int noise_rows, uint64_t seed, uint64_t sample_id_base, uint32_t draw,
                     float* out, double* gain_out, void* stream);

/* ---- Scoring (ABI 12, additive; no reference counterpart beyond the one-timestep estimator, compute_loss with t0_always = True,
 * diffusion_qm9.py:530-699): the variational bound of GIVEN molecules with every term of a list evaluated, in the device loop.
 * For normalised data xh [B,N,D] and a term t in 1 .. T (s = t - 1):
 *     eps_t = combined noise (masked, x part mean-free over the valid nodes; draw layout at hd_noise),
 *     z_t = alpha_t xh + sigma_t eps_t,   eps^_t = hd_egnn_forward(z_t, tau[t]),   e_t = sum_{nodes, columns} (eps_t - eps^_t)^2,
 *     acc[b] += w_t e_t,   w_t = 0.5 expm1(gamma_t - gamma_s)   (= 0.5 (SNR(gamma_s - gamma_t) - 1), the reference's weight)
 * and nll = kl_prior + (T / K) fp32(acc) + neg_log_constants + L_0 - delta_log_px, L_0 = -log p(x, h | z_0) with its own draw eps_0 -
 * the reference's estimator with its random t replaced by the K listed ones (K = T: the full bound, exact in t, one eps per term).
 * acc is a DOUBLE per molecule in device memory: one thread adds the terms in list order, node sums run in a fixed order, no atomics; a
 * molecule's score depends on its global id, its mask, the weights, the schedule and its data - not on the batch, the order of the
 * terms or how their range was split into calls.
 *
 * hd_set_nll_terms uploads the list next to the plain schedule, which must be set (it supplies T and tau) and whose replacement needs
 * a new upload here (HD_E_STATE otherwise).  Host arrays: t_idx [K] grid indices in 1 .. T, coef4 K rows {alpha_t, sigma_t, w_t, 0}. */
int hd_set_nll_terms(hd_handle* h, int K, const int* t_idx, const float* coef4);
/* Terms k = k_lo ... k_hi-1 of the list: acc[B] (device doubles, zeroed by the caller before the first term) += w_t e_t.
 *   xh           device [B,N,D] normalised data; context as in hd_egnn_forward (passed through unchanged)
 *   raw_x/raw_h  device [(k_hi-k_lo), B, N, 3|F] normals per term, indexed by list position (first = k_lo), or NULL = the generator
 *   err_terms    NULL, or device [K][B]: row k receives e_t of term k (rows outside k_lo .. k_hi-1 are untouched)
 *   use_graph    ONE captured term per topology, whatever K, replayed k_hi - k_lo times: the position lives in device memory and the
 *                captured kernels read time, row and draw through the uploaded tables.  Cached with the topology and rebuilt when the
 *                terms, seed, weights, schedule or noise arguments change (hd_nll_graph_builds counts the instantiations; -1: null
 *                topology); use_graph = 0 gives the same bits.  Stream-ordered, no host synchronisation in steady state.
 * Restrictions (HD_E_INVALID): noise_rows = B, mol_shape < 0 or = N (no pocket rows), N * D floats within one workgroup's LDS. */
int hd_nll_terms(hd_handle* h, hd_topology* topo, const float* xh, const float* context, int mol_shape, int k_lo, int k_hi,
                 const float* raw_x, const float* raw_h, int noise_rows, uint64_t seed, uint64_t sample_id_base, int use_graph,
                 double* acc, float* err_terms, void* stream);
long long hd_nll_graph_builds(const hd_topology* topo);
/* nll[B] from acc: draws eps_0 (raw_x/raw_h device [B,N,3|F], or NULL = the generator at draw 0), z_0 = alpha_0 xh + sigma_0 eps_0, the
 * network at tau[0], then one kernel for kl_prior, the constants, L_0 and the sum.  K = number of terms acc holds (T / K scales them).
 *   consts7      host {alpha_0, sigma_0, gamma_0, gamma_T, norm_values[2], norm_biases[2], log(norm_values[0])}
 *   int_nf / cont_nf  integer / continuous feature columns of the t = 0 likelihood, as in hd_vlb_loss_forward (5 / 3 or 3 / 0).
 * Restrictions of hd_nll_terms. */
int hd_nll_finish(hd_handle* h, hd_topology* topo, const float* xh, const float* context, int mol_shape, const float* raw_x,
                  const float* raw_h, int noise_rows, uint64_t seed, uint64_t sample_id_base, int K, const float* consts7, int int_nf,
                  int cont_nf, const double* acc, float* nll, void* stream);

/* ---- Fragment-constrained sampling ("inpainting"; ABI 12, additive; no reference counterpart): sample the free nodes of a
 * molecule around fragments whose positions and features are known, by the replacement method of score-based models, optionally with
 * RePaint-style resampling.  For s = s_hi-1 ... s_lo, t = s + 1, and round j = 0 .. resamplings-1:
 *   1. z_gen = the posterior step of the plain loop (network call at tau[t], noise, masked mean removal), unchanged;
 *   2. z_kn  = alpha_s xh_known + sigma_s e_kn on the fixed rows (e_kn standard normal per node and component);
 *   3. per molecule c = mean_fixed(z_gen.x) - mean_fixed(z_kn.x); z_s = where(fixed, z_kn + [c, 0], z_gen), then the masked mean
 *      removal of the x part the plain step ends with.  A molecule without fixed nodes keeps z_gen bit for bit;
 *   4. if j < resamplings-1: z_t = alpha_t|s z_s + sigma_t|s e_jump (e_jump: combined noise, masked, x part mean-free over the valid
 *      nodes) and back to 1 at the same (s, t).
 * Noise comes from the counter-based generator only, in the draw layout documented at the noise entry point above: a sample's bits
 * depend on its global id, its masks, the weights and its known values - not on the batch it runs in.  Sums over a molecule's nodes
 * run in a fixed order (no atomics).
 *
 * Schedule rows for the loop: host array of T rows {alpha_s, sigma_s, alpha_t_given_s, sigma_t_given_s} for s = 0..T-1 (t = s+1), from the
 * same gamma grid as the plain schedule; T must equal the T of the last schedule upload, and a new plain schedule needs a new upload here.
 * They become the inpainting rows of the handle's every-step tables (hd_set_schedule). */
int hd_set_inpaint_schedule(hd_handle* h, int T, const float* coef4);
/* The arguments of the plain loop plus
 *   fixed_mask   device bytes [B*N] (0 = free), a subset of the node mask (rows outside it are ignored);
 *   xh_known     device [B,N,D] NORMALISED known positions and features (rows outside fixed_mask are ignored);
 *   resamplings  r >= 1.
 * Restrictions (HD_E_INVALID): raw_x / raw_h must be NULL, noise_rows = B, mol_shape < 0 or = N (no pocket rows).
 * This is hd_sample_path_inpaint's loop on the handle's every-step tables (transitions T - s_hi ... T - s_lo - 1), with a graph slot
 * of its own.  use_graph: one captured step (all its rounds) per topology, cached like the plain loop's and rebuilt when resamplings,
 * seed, weights or schedule change; use_graph = 0 gives the same bits.  Stream-ordered, no host synchronisation in steady state. */
int hd_sample_loop_inpaint(hd_handle* h, hd_topology* topo, float* z, const float* context, int mol_shape,
                           int s_hi, int s_lo, const float* raw_x, const float* raw_h, int noise_rows,
                           uint64_t seed, uint64_t sample_id_base, int use_graph, const uint8_t* fixed_mask,
                           const float* xh_known, int resamplings, void* stream);
/* Behind the final decode, in DATA units (after unnormalize): on the fixed rows hfeat = h_known exactly and
 * x = x_known + (mean_fixed(x) - mean_fixed(x_known)), so the returned fragments are a pure translation of the given ones.
 * x, x_known device [B,N,3]; hfeat, h_known device [B,N,F]; other rows and molecules without fixed nodes are untouched. */
int hd_inpaint_decode_fix(hd_handle* h, hd_topology* topo, const uint8_t* fixed_mask, const float* x_known,
                          const float* h_known, float* x, float* hfeat, void* stream);
/* PARTIAL INPAINTING (additive): positions or features alone, per feature channel.  Two masks replace the single one, both subsets
 * of the node mask (a set byte on a masked row is ignored): fx[n] "the position of node n is known" and fh[n][c] "feature channel c
 * of node n is known"; the whole-node call is fx[n] = fh[n][.] = fixed[n].  Steps 1 and 4 above are unchanged; 2 - 3 become
 *   2'. element e = n D + c is REPLACED if c < 3 and fx[n], or c >= 3 and fh[n][c - 3]; a replaced element becomes
 *       alpha_s known[e] + sigma_s normal(seed, id, draw, e) - today's draw and element index (stream k = 1 of the inpainting layout);
 *       an element that is not replaced does not use its normal;
 *   3'. with Fx the molecule's valid nodes with fx: |Fx| > 0 - c = mean_Fx(z_gen.x) - mean_Fx(z_kn.x) is added to the replaced
 *       positions, then the masked mean over all valid nodes is removed, in the order of the whole-node form;  |Fx| = 0 - the
 *       position part of z_gen keeps its BITS (no frame, and z_gen.x is mean-free already).  Nothing replaced: z_gen bit for bit.
 * Masks that coincide give the bits of the whole-node form.  Position components of a node are known together (no per-axis mask).
 * With the restraints in the known fragments' frame (hd_restraint_frame 1) "the valid fixed nodes F" is Fx: a node with known
 * features and a free position is a free node and is pushed; |Fx| = 0 gives tau = 0 and the plain update.
 * hd_inpaint_parts: attach (fixed_h: device bytes [B*N*F], copied in stream order into a buffer the topology owns) or detach (NULL).
 *   While attached, the fixed_mask of hd_sample_loop_inpaint / hd_sample_path_inpaint / hd_sample_path_guided means "position known"
 *   and the attached bytes "channel known"; calls that do not inpaint ignore the attachment.  Whether parts are attached is part of
 *   the graph key: attaching or detaching rebuilds the captured transition once, other mask contents replay it, and a whole-node
 *   call after a detach gives the bits of a topology that never had parts.  Every restriction of the inpainting loops stays.
 * hd_inpaint_replace: steps 2' - 3' once, in place on z [B][N][D], with the host values alpha_s / sigma_s and the generator's
 *   (seed, sample_id_base + row, draw); fixed_x u8 [B*N]; fixed_h u8 [B*N*F], or NULL for the whole-node form (fixed_x = fixed).
 * hd_inpaint_decode_fix_parts: hd_inpaint_decode_fix with the two masks - hfeat = h_known exactly on the replaced channels,
 *   x = x_known + (mean_Fx(x) - mean_Fx(x_known)) on Fx, everything else untouched. */
int hd_inpaint_parts(hd_handle* h, hd_topology* topo, const uint8_t* fixed_h, void* stream);
int hd_inpaint_replace(hd_handle* h, hd_topology* topo, float* z, const uint8_t* fixed_x, const uint8_t* fixed_h,
                       const float* xh_known, float alpha_s, float sigma_s, uint64_t seed, uint64_t sample_id_base, uint32_t draw,
                       void* stream);
int hd_inpaint_decode_fix_parts(hd_handle* h, hd_topology* topo, const uint8_t* fixed_x, const uint8_t* fixed_h,
                                const float* x_known, const float* h_known, float* x, float* hfeat, void* stream);

/* ---- Training primitives (the handle's hd_config.precision must be 0; the fp16x3 contractions are chosen per call below).
 * One "edge layer" is the part of a GCL / EquivariantUpdate that works on edges (egnn_new.py:35-56 / :91-104 with the
 * first Linear factorised): per unmasked edge (i, j)
 *     pre1 = A_i + B_j + |x_i - x_j|^2 w_r + |x0_i - x0_j|^2 w_d,   P = SiLU(pre1),   M = SiLU(W2 P + b2),
 *     GCL:   out_i = sum_j M sigmoid(wa.M + ba) / normalization_factor                          [M][H]
 *     COORD: out_i = sum_j u_ij tanh(wa.M) coords_range / normalization_factor  (xyz, 4th = 0)   [M][4]
 * with AB = [A | B] [M][2H] the node-level halves of the first Linear (computed by the caller, e.g. with a library
 * GEMM), x / x0 [M][4] the coordinates at block start / network input, M = active nodes, rows in the topology's
 * compact node order (hd_topology_nodes).  Weights are DEVICE pointers in state_dict layout: wrd [2][H] = the two
 * distance columns of the first Linear, W2 [H][H], b2 [H], wa [H], ba [1] (NULL: no attention bias).  The node-level Linears around an edge layer are plain GEMMs:
 * hierdiff_amd/training.py runs them on hd_gemm_f32 below (forward, dX and split-K dW; no BLAS-library kernel in a step). */
int hd_topology_nodes(const hd_topology* t, int* node_of /* host, `active nodes` ints: flat index b*N + n */);
/* The same order for a device consumer: `active nodes` int64 flat indices written to DEVICE memory in stream order. */
int hd_topology_nodes_device(hd_topology* t, long long* index, void* stream);
int hd_edge_layer_forward(hd_handle* h, hd_topology* topo, int coord, const float* AB, const float* x,
                          const float* x0, const float* wrd, const float* W2, const float* b2, const float* wa,
                          const float* ba, float* out, void* stream);
/* The same forward / backward with two per-call choices (hd_edge_layer_forward / _backward are the (precision 0, pre2 NULL) case).
 * (1) Keep the second-layer pre-activations instead of recomputing them: hd_edge_layer_save_rows = rows of a [rows][hidden_nf] fp32
 * buffer the forward of this topology can fill (the table's rows plus one spare tile; 0: the batch is small enough for the
 * column-split edge kernels, which keep their faster forward - pass pre2 = NULL and the backward recomputes).
 * hd_edge_layer_forward_s with pre2 != NULL writes W2 P + b2 of every edge row into it (accumulator order per 32-row tile, opaque to
 * the caller; 228 MB per layer at B = 256, N = 30, H = 256 - sized for this GPU's HBM, not for a 16 GB card);
 * hd_edge_layer_backward_s with the same buffer runs stage A as an element-wise kernel over it (no weight stream, no matrix
 * instruction).  Same results to the bit as the recomputing path (tests/test_gpu_edge_layer.py, tests/test_gpu_training.py).
 * (2) precision: 0 = exact fp32; 3 = "fp16x3" (hidden_nf >= 128; narrower layers run the fp32 kernels): the sampler's two-way FP16
 * split in the training path - the reference trains with apex O2 (endiffusion/conf/trainer/default.yaml:4-5); here the forward
 * contraction (the fp16x3 edge kernel on the unscaled parameters; images, image scale and row ranges made on the device per call),
 * stage B's dP = G2 W2 (operand rows ranged by their exact maxima, which stage A leaves in f16ws) and dW2 (hd_dw2_f16) run on the
 * matrix cores proper, fp32-accurately, while everything around them stays exact fp32.  It exists only together with the kept pre2
 * (whose spare tile carries the image scalars from the forward to the backward call): hd_edge_layer_backward_s(precision 3) needs
 * the pre2 of a precision-3 forward and f16ws (hd_edge_layer_f16ws_floats floats, *n_wg = the number of per-workgroup maxima
 * hd_dw2_f16 reads at f16ws + 4 and f16ws + 4 + n_wg); where hd_edge_layer_save_rows(.., 3) is 0 the caller runs the layer in
 * precision 0.  (precision 2 = "bf16x6", the _p entry points and hd_dw2_x6 existed up to ABI 11.) */
long long hd_edge_layer_f16ws_floats(hd_handle* h, hd_topology* topo, int* n_wg);
int hd_dw2_f16(int device, int rows, int H, const float* G2, const float* P, const float* gmax, const float* pmax, int n,
               float* dW2, int ldc, float* ws, long long ws_floats, void* stream);
long long hd_edge_layer_save_rows(hd_handle* h, hd_topology* topo, int precision);
int hd_edge_layer_forward_s(hd_handle* h, hd_topology* topo, int coord, int precision, const float* AB, const float* x,
                            const float* x0, const float* wrd, const float* W2, const float* b2, const float* wa,
                            const float* ba, float* out, float* pre2, void* stream);
int hd_edge_layer_backward_s(hd_handle* h, hd_topology* topo, int coord, int precision, const float* AB, const float* x,
                             const float* x0, const float* wrd, const float* W2, const float* b2, const float* wa,
                             const float* ba, const float* gout, const float* pre2, float* f16ws, float* G2, float* P, float* G1, float* escal,
                             float* colpart, float* bapart, float* b2part, float* wrdpart, float* dAB, float* dx, float* dx0,
                             void* stream);
/* Backward of hd_edge_layer_forward given gout = dL/d(out).  Per-edge activations are recomputed; the caller provides
 * workspaces G2, P, G1 [rows][H], escal [rows][8], colpart, b2part [tiles][H], wrdpart [tiles][2][H], bapart [tiles]
 * (rows / tiles from hd_topology_layout's counts, tiles rounded up to a multiple of 4).  Written: dAB [M][2H],
 * dx, dx0 [M][4] and, for the caller's reductions over all edge rows,
 *     G2 = dL/d(W2 P + b2),  P                          =>  dW2 = G2^T P              (one dense GEMM, K = rows),
 *     per-tile partial sums                             =>  db2 = colsum(b2part),  d(wa) = colsum(colpart),
 *                                                           d(ba) = sum(bapart),
 *                                                           d(w_r), d(w_d) = colsum(wrdpart[:, 0]), colsum(wrdpart[:, 1]);
 * G1 = dL/d(pre1) is the operand of the two CSR sums behind dAB and is left in the workspace.  escal, one 8-float record per edge
 * row: {dL/du_x, dL/du_y, dL/du_z, dL/dphi, dL/d(radial), dL/d(d0), -, -} with u the unit direction and phi = wa.M of a coordinate
 * layer and d(radial), d(d0) the paths through pre1; [0:4] are written (and read) in coordinate layers only, [6:8] never.  Every
 * other row of every array is written - zeros on the padding rows of the table - so no workspace needs clearing
 * (tests/test_gpu_edge_layer.py). */
int hd_edge_layer_backward(hd_handle* h, hd_topology* topo, int coord, const float* AB, const float* x,
                           const float* x0, const float* wrd, const float* W2, const float* b2, const float* wa,
                           const float* ba, const float* gout, float* G2, float* P, float* G1, float* escal, float* colpart,
                           float* bapart, float* b2part, float* wrdpart, float* dAB, float* dx, float* dx0, void* stream);

/* ---- One node step of the forward on its own (ABI 12, additive): a test and diagnosis primitive, nothing on the hot path calls it.
 * The node side of hd_egnn_forward between two edge kernels, run by the function the forward itself calls, in the handle's precision
 * mode and on the path the forward takes at this topology's size:
 *     agg_i = (sum of the node's rows of `part`, pstart[i] ... pstart[i + 1] - 1) / normalization_factor   (N with 'mean')
 *     T = SiLU([h | agg] W3^T + b3),   h' = (h + T W4^T + b4) * node_mask,   AB_q = h' [W1a_q | W1b_q]^T + [b1_q | 0]
 * layer == -1: the AB-only step after the embedding (h' = h; AB of GCL 0; `part` may be NULL).  0 <= layer < n_layers *
 * inv_sublayers: the update with the node model of GCL layer = i * inv_sublayers + j, and the AB of what follows it in the forward:
 * the next sub-layer (j + 1 < inv_sublayers), else the block's coordinate layer (ab0) and - for i + 1 < n_layers - the next block's
 * first GCL (ab1): ab1 is required exactly when the step writes two images.
 * All pointers are DEVICE pointers, rows in the topology's compact node order (hd_topology_nodes), M = active nodes:
 * h_in, h_out [M][H] (may be the same pointer), part [parts][H] (parts = info6[5] of hd_topology_info, a node's range from the pstart
 * of hd_topology_layout), ab0, ab1 [M][2H], abmax0, abmax1 [M][2] or NULL: {max_k |A_r[k]|, max_k |B_r[k]|}, the row maxima the
 * next edge kernel of this handle would read - the node kernels' own where they write them, k_ab_rowmax's where the forward
 * launches that (precision 3 below width 128); a handle of precision 0 keeps none and refuses the pointer.
 * A handle of precision 3 runs its edge model in the domain scaled by c = -log2(e) (hd_set_weights folds c into the packed weights,
 * one rounding per weight): there `part` is what its edge kernels leave, c x the neighbour sums, and ab* / abmax* are c x the AB above,
 * what its edge kernels read; h_in and h_out are unscaled in every precision.
 * The call copies h_in and part into the topology's buffers in stream order, runs the step and copies the results out; *path
 * (host) receives the path taken: 0 three-launch fp16x3 chain, 1 three-launch fp32 chain, 2 fused kernel, 3 the 16-row GEMM chain.
 * HD_E_INVALID (and no launch): null handle, topology or tensor, layer out of range, a topology of another handle, ab1 missing,
 * abmax given in precision 0; HD_E_STATE: weights not set (tests/test_gpu_node_step.py). */
int hd_node_step(hd_handle* h, hd_topology* topo, int layer, const float* h_in, const float* part, float* h_out,
                 float* ab0, float* ab1, float* abmax0, float* abmax1, int* path, void* stream);

/* ---- Stage-2 layer: E_GCL forward (/root/reference/models/egnn/gcl.py:9-205), exact fp32.
 * The layer of the edge-denoise / refine models: messages from [h_row; h_col; radial; edge_attr; context], optional
 * attention gate, coordinate update and node update aggregated over the RECEIVING index `col`, optional update of the
 * H-wide edge features.  agg = 'sum', node_attr = None, act_fn = SiLU. */
typedef struct hd_egcl hd_egcl;
typedef struct hd_egcl_graph hd_egcl_graph;
typedef struct hd_egcl_config {        /* E_GCL.__init__ arguments (gcl.py:19) */
    int32_t hidden_nf;                 /* input_nf == output_nf == hidden_nf: 32, 64, 128 or 256 */
    int32_t edges_in_d;                /* hidden_nf (edge features) or < 32 (scalar edge attributes, e.g. 1) */
    int32_t context_nf;
    int32_t attention, tanh, coord_update, edge_update, recurrent;
    float coords_range;
    int32_t geo;                       /* 1: the message model sees 1 / radial^2 instead of radial (gcl.py:170-175); the coordinate and
                                          edge models keep radial.  An edge list with self edges then carries inf / NaN, as in the reference */
} hd_egcl_config;
int hd_egcl_create(const hd_egcl_config* cfg, int device, hd_egcl** out);
int hd_egcl_destroy(hd_egcl* g);
long long hd_egcl_weight_count(const hd_egcl* g);
/* Parameters flattened in state_dict registration order: mes_mlp.{0,2}, [edge_mlp.{0,2}], node_mlp.{0,2},
 * [coord_mlp.{0,2}], [att_mlp.0] (weight then bias each; coord_mlp.2 has no bias). */
int hd_egcl_set_weights(hd_egcl* g, const float* blob, long long n, int on_device, void* stream);
/* Edge list (HOST int32 arrays row, col [E], node ids < M) + workspaces; reusable across layers of the same width. */
int hd_egcl_graph_create(hd_egcl* g, const int* row, const int* col, int M, int E, hd_egcl_graph** out);
int hd_egcl_graph_destroy(hd_egcl_graph* t);
/* (h_out [M][H+ctx], x_out [M][3], edge_attr_out [E][H]) = E_GCL.forward(h [M][H+ctx], edges, x [M][3], edge_attr [E][De],
 * node_mask [M] or NULL, edge_mask [E] or NULL); all device fp32; edge_attr_out only with edge_update.  A graph with E = 0 is
 * valid (the node model on a zero aggregate): its zero-length edge tensors - edge_attr, edge_attr_out, and edge_mask,
 * dedge_attr_out, dedge_attr of the calls below - are never read or written and may be NULL. */
int hd_egcl_forward(hd_egcl* g, hd_egcl_graph* t, const float* h, const float* x, const float* edge_attr,
                    const float* node_mask, const float* edge_mask, float* h_out, float* x_out, float* edge_attr_out,
                    void* stream);
/* Training (ABI 12, additive): the same forward, which also keeps what the backward needs in a CALLER-OWNED buffer `saved` of
 * hd_egcl_saved_floats(g, M, E) device floats (the graph's workspaces are overwritten by the next call on the same graph, and a model
 * applies one layer several times per forward).  h_out / x_out / edge_attr_out are the bits of hd_egcl_forward. */
long long hd_egcl_saved_floats(const hd_egcl* g, int M, int E);
int hd_egcl_forward_train(hd_egcl* g, hd_egcl_graph* t, const float* h, const float* x, const float* edge_attr,
                          const float* node_mask, const float* edge_mask, float* h_out, float* x_out, float* edge_attr_out,
                          float* saved, void* stream);
/* Backward of hd_egcl_forward_train with the same inputs and its `saved` buffer, given dh_out [M][H+ctx], dx_out [M][3] and
 * dedge_attr_out [E][H] (each may be NULL = zero).  Writes dh [M][H+ctx], dx [M][3], dedge_attr [E][De] (NULL: not wanted) and
 * dweights, the gradient of every parameter in the layout of hd_egcl_set_weights (state_dict order).  Exact fp32: the dense
 * products on the training GEMM (hd_gemm_f32), sums over edges in a fixed order (CSR over row / col, split-K in slab order) -
 * deterministic.  The mask tensors get no gradient.  The backward reads the weights of the last hd_egcl_set_weights. */
int hd_egcl_backward(hd_egcl* g, hd_egcl_graph* t, const float* h, const float* x, const float* edge_attr,
                     const float* node_mask, const float* edge_mask, const float* saved, const float* dh_out,
                     const float* dx_out, const float* dedge_attr_out, float* dh, float* dx, float* dedge_attr,
                     float* dweights, void* stream);

/* ---- Refine model (Node2Vec, models/model_refine.py of the reference; ABI 12, additive), exact fp32, deterministic.
 * Input gather: out [M][ldo] columns off_v.. = Ev [nv][H] row v[m], columns off_s.. = Es [ns][H] row size[m] (v, size: device int64
 * [M]).  An id outside its table writes zeros and sets *bad = 1 (a device int the caller zeroes and reads); it is never dereferenced.
 * Backward: dEv [nv][H] and dEs [ns][H] = per-id sums of the same columns of dout, rows added in ascending order; the row of an
 * id that never occurs is zero.  M = 0 is valid (the backward writes zero tables); v, size, out / dout may then be NULL. */
int hd_refine_embed_forward(int device, const long long* v, const long long* size, int M, int H, int nv, int ns, const float* Ev,
                            const float* Es, float* out, int ldo, int off_v, int off_s, int* bad, void* stream);
int hd_refine_embed_backward(int device, const long long* v, const long long* size, int M, int H, int nv, int ns, const float* dout,
                             int ldo, int off_v, int off_s, float* dEv, float* dEs, void* stream);
/* Edge attribute on an E_GCL edge graph: ea [E] = |x[row] - x[col]|^2 (x [M][3]); backward dx [M][3] from dea [E], summed per
 * node over the graph's CSR lists (first the edges the node sends, then those it receives).  E = 0: ea / dea may be NULL, dx = 0. */
int hd_sqdist_forward(hd_egcl_graph* t, const float* x, float* ea, void* stream);
int hd_sqdist_backward(hd_egcl_graph* t, const float* x, const float* dea, float* dx, void* stream);
/* Size-restricted softmax head.  logits [B][ld] (first ncols columns); candidate sets cand_ids (device int32, set s at
 * [cand_off[s], cand_off[s + 1]), ids unique within a set) with cand_off [nsets + 1]; set_idx [B], target [B] device int32.
 * Forward: logp [B] = log-softmax over the row's set at the target, hit [B] = (argmax over the set == target), topk [B][k] the k
 * best candidate ids (0 <= k <= 16; value descending, ties to the lower position in the set; -1 past the set's size).  *err
 * (device int, zeroed by the caller): 1 a target outside its set, 2 a set index out of range, 3 a candidate id >= ncols.
 * Backward: dlogits [B][ld] = dloss[b] (softmax over the set - onehot(target)) on the set's columns, 0 on the other ncols columns. */
int hd_cand_xent_forward(int device, int B, const float* logits, int ld, int ncols, const int* cand_ids, const int* cand_off, int nsets,
                         const int* set_idx, const int* target, int k, float* logp, int* hit, int* topk, int* err, void* stream);
int hd_cand_xent_backward(int device, int B, const float* logits, int ld, int ncols, const int* cand_ids, const int* cand_off, int nsets,
                          const int* set_idx, const int* target, const float* dloss, float* dlogits, void* stream);

/* y [M][ldy] (first N columns) = act(x [M][ldx] (first K columns) . W [N][K]^T + b [N] or NULL); device fp32, any M, K, N.
 * act: 0 none, 1 SiLU, 2 sigmoid.  The small dense layers around the E_GCL chains of the stage-2 model - torch.nn.Linear in
 * /root/reference/models/edge_denoise.py:29-33 (feature / edge / node embeddings) and :55-57 (focal / edge / node prediction
 * heads, Linear + SiLU + Linear [+ Sigmoid]).  One fmaf chain over k per output element, k ascending: the kernel reads four
 * floats at a time when K and ldx are multiples of 4 and both x and W are 16-byte aligned, one at a time otherwise (a view at an
 * odd float offset, a padded ldx) - same chain, same bits either way.  M = 0 is accepted and writes nothing. */
int hd_linear(int device, const float* x, int M, int K, int ldx, const float* W, const float* b, int N, int act,
              float* y, int ldy, void* stream);

/* General exact-fp32 GEMM of the training path (csrc/k_tgemm.hpp): C [M][ldc] = epi(sum_k A(m,k) B(k,n)) with
 * A(m,k) = A[m a_m_stride + k a_k_stride], B(k,n) = B[k b_k_stride + n b_n_stride], one unit stride per operand - the
 * node-level nn.Linear modules of the EGNN (egnn_new.py:17-33,76-89,172-173) under autograd: forward Y = X W^T + b,
 * backward dX = dY W and dW = dY^T X (diffusion_qm9.py:774-777 -> torch.autograd), and the dense reduction over all edge rows
 * dW2 = G2^T P of hd_edge_layer_backward.  epi: 0 C = acc + bias; 1 C = acc + bias, C2 = SiLU(C); 2 C = (aux + acc + bias) *
 * row_mask[m] (row_mask may be NULL); 3 C = acc * SiLU'(aux).  bias [N] or NULL.  split_k > 1 (epi 0 only): K is cut into
 * slabs whose partial results go to ws ([slabs][M][N] floats, + [slabs][M] when colsum is given) and are added in slab order
 * (deterministic); colsum [M] (any split_k, ABI 10: also 1 - no workspace then) receives sum_k A(m,k) (the bias gradient of
 * dW = dY^T X; A must be m-contiguous).  The slab count actually used is ceil(K / (32 * ceil(K / split_k / 32))) <= split_k. */
int hd_gemm_f32(int device, int M, int N, int K, const float* A, long long a_m_stride, long long a_k_stride,
                const float* B, long long b_k_stride, long long b_n_stride, float* C, int ldc, const float* bias,
                int epi, const float* aux, const float* row_mask, float* C2, int split_k, float* ws,
                float* colsum, void* stream);

/* (hd_dw2_f16, declared with the edge-layer functions above: dW2 [H][ldc] = G2^T P over `rows` edge rows - G2, P [rows][H] as
 * hd_edge_layer_backward_s leaves them, rows a multiple of 32, H = 128 or 256 - in fp16x3 arithmetic, csrc/k_dw2.hpp: the
 * fp32-accurate form of the one dense reduction over all edge rows.  ws: ws_floats >= H * H device floats; the product is cut into
 * min(256, ws_floats / H^2, rows / 128) slabs whose partial results are added in a fixed order: deterministic.) */
/* The variational training loss around the network call as one kernel per direction (round 5; reference: compute_loss with
 * t0_always = False, diffusion_qm9.py:530-673, and what it calls - compute_error :160-172, kl_prior :206-239, the log constants
 * :241-262, log_pxh_given_z0_without_constants :460-528).  All tensors fp32 on the device: net / zt / xh / eps [B][N][D] (network
 * output, noised input, normalised data [x | h], noise), nm [B][N], gam [4][B] = gamma at (s, t, 0, 1), t_int [B].  int_nf / cont_nf:
 * integer / continuous feature columns of the t = 0 likelihood (5 / 3 for node_coarse_type 'prop', 3 / 0 otherwise); l2_train: the
 * `l2` training loss; T timesteps; nv2 / nb2 = norm_values[2] / norm_biases[2]; log_nv0 = log(norm_values[0]).
 * All tensors are dense and contiguous, and masked-out nodes of net / eps / xh must be zero (the sums run over every node).
 * forward: loss [B] (= nll per molecule), err [B] (= the `error` of the reference's info dict).
 * backward: given gout = dL/d(loss) [B]: dnet, dzt [B][N][D] and dgam [4][B] (the schedule network is trained).
 * hd_vlb_zt: z_t = sqrt(sigmoid(-g_t)) xh + sqrt(sigmoid(g_t)) eps (dzt = NULL), or dgt[b] = d/dg_t of that against dzt. */
int hd_vlb_loss_forward(int device, int B, int N, int D, int int_nf, int cont_nf, int l2_train, float T, float nv2, float nb2,
                        float log_nv0, const float* net, const float* zt, const float* xh, const float* eps, const float* nm,
                        const float* gam, const float* t_int, float* loss, float* err, void* stream);
int hd_vlb_loss_backward(int device, int B, int N, int D, int int_nf, int cont_nf, int l2_train, float T, float nv2, float nb2,
                         float log_nv0, const float* net, const float* zt, const float* xh, const float* eps, const float* nm,
                         const float* gam, const float* t_int, const float* gout, float* dnet, float* dzt, float* dgam, void* stream);
int hd_vlb_zt(int device, int B, int ND, const float* xh, const float* eps, const float* gt, float* zt, const float* dzt, float* dgt,
              void* stream);
/* Layout of the first edge Linear for the edge layer, one launch (round 5: a training step at the reference's batch size is bound
 * by the NUMBER of launches): W1 [H][2H + 2] (state_dict layout, columns h_row | h_col | radial | d0), b1 [H] -> Wst [2H][H] (the two
 * node halves stacked: AB = h Wst^T + bst), bst [2H] = [b1 | 0], wrd [2][H] (hd_edge_layer_forward's wrd).  dir 1: the way back for
 * the gradient - W1 receives dW1 assembled from Wst = dWst and wrd = dwrd (b1 / bst unused). */
int hd_edge_prep(int device, int H, int dir, float* W1, const float* b1, float* Wst, float* bst, float* wrd, void* stream);
/* Column sums of n <= 4 device arrays src[i] [rows][width[i]] into dst[i] [width[i]] in two launches, rows added in a fixed
 * order (32 ascending row ranges, then the ranges ascending): the reductions hd_edge_layer_backward leaves to its caller
 * (db2, d(wa), d(w_r) / d(w_d), d(ba) from the per-tile partial sums).  src / width / dst are HOST arrays of n entries;
 * ws: 32 * sum(width) device floats. */
int hd_colsum_f32(int device, int rows, int n, const float* const* src, const int* width, float* const* dst, float* ws,
                  void* stream);

/* 64-bit content digest of n device tensors of 32-bit words (the parameters a packed image was made from): the Python wrapper
 * compares it with the digest taken when it last called hd_set_weights / hd_set_schedule / hd_egcl_set_weights, so that a writer
 * which bumps no version counter (a fused optimizer, `.data` writes, an external kernel) can never leave the inference path on a
 * stale image.  The reference has no counterpart: it evaluates its modules in place (en_dynamics.py:49-122).
 * ptrs_dev [n] device pointers, prefix_dev [n + 1] word offsets (prefix_dev[n] == total), both DEVICE arrays; state_dev: two
 * device uint64 that are ZERO on entry (the kernel leaves them zero again).  One launch - the last workgroup publishes the sum to a
 * pinned host word - and one wait for `stream`.  The value is independent of the launch geometry. */
int hd_params_digest(int device, const void* const* ptrs_dev, const long long* prefix_dev, int n, long long total,
                     unsigned long long* state_dev, unsigned long long* digest_host, void* stream);

/* Host implementation of the library's normal generator (same bits as the device one up to libm
 * round-off); used by tests and by callers that want to reproduce a draw on the CPU. */
float hd_philox_normal_host(uint64_t seed, uint64_t sample_id, uint32_t draw, uint32_t index);
/* Host twin of the uniform the steering stage draws (exactly the device's bits: integer arithmetic and one exact conversion): words
 * 2 and 3 of the counter block (index / 2, draw, sample_id) - the normals take words 0 and 1 - 26 bits each, in double, in (0, 1). */
double hd_philox_uniform_host(uint64_t seed, uint64_t sample_id, uint32_t draw, uint32_t index);

/* Kernel timing of the most recent hd_egnn_forward when profiling is enabled: per-kernel-family
 * accumulated milliseconds measured with HIP events on the caller's stream.
 * families: 0 edge (GCL+coord), 1 node GEMMs, 2 other.  `on` is a bitmask of the families to bracket
 * (1 = edge kernels only, 7 = all, 0 = off), optionally OR-ed with (stride << 8) to bracket only every
 * stride-th forward; enabling inserts event records only.  Launches replayed from a hipGraph are not
 * bracketed. */
int hd_profile_enable(hd_handle* h, int on);
int hd_profile_read(hd_handle* h, double* ms3, long long* launches3);

/* Measurement aid (no reference counterpart; bench.py's `roofline.sustained`): the rate at which THIS chip, under its power budget,
 * issues one matrix instruction when every SIMD streams it from register operands at the edge kernels' occupancy (two wavefronts per
 * SIMD, eight accumulators, operands taken from `in1024` - pass random data, zeros clock higher).  kind 0: v_mfma_f32_32x32x2_f32,
 * 1: v_mfma_f32_32x32x16_f16.  `scratch`: 2 * 256 * (number of CUs) device floats.  Runs the loop twice
 * (warm-up, timed with HIP events on `stream`) and waits for it.  *ns_per_mfma_per_simd = elapsed / (MFMAs issued per SIMD). */
int hd_mfma_probe(int device, int kind, const float* in1024, float* scratch, int iters, double* ns_per_mfma_per_simd, void* stream);

/* Debug aid (no reference counterpart), live only in a measurement build of the library
 * (python -m hierdiff_amd.build --debug-kernels; the product build returns 0): per-wave cycle stamps of the
 * handle's most recent traced edge-kernel launch (environment HD_ABLATE with bit 16 set at hd_create; H = 256,
 * GCL variant).  32 int64 per workgroup = 4 waves x {start|HW_ID<<48, loop start|XCC_ID<<48, loop end,
 * end, 3 epilogue stamps, segments}.  Returns the number of workgroups copied (0 if nothing was traced). */
int hd_debug_edge_trace(hd_handle* h, long long* out, int max_wg);

#ifdef __cplusplus
}
#endif
#endif /* HIERDIFF_HIP_H */
