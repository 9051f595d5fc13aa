/* tipk.h -- C ABI of libtipk.so: the MI355X (gfx950) kernels behind the TIP hot path.
 *
 * The reference (NYXFLOWER/TIP) has no FFI/plugin layer for this path: its boundary is the Python
 * `nn.Module` surface of `src/layers.py`, and all device arithmetic is delegated to torch, PyG 2.0.1
 * and torch-scatter 2.0.8.  Each entry point below therefore names the reference call site whose
 * implicit torch/PyG kernels it replaces (paths relative to the reference root; K-numbers are
 * SURVEY.md section 2.1).  `tip_amd/_lib.py` binds every symbol with ctypes; INTEGRATION.md shows
 * the stub a reference maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless marked host; fp32 values, int32 indices (the Python
 *     side narrows the reference's int64 tensors once, when it builds a plan);
 *   - `stream` is a hipStream_t (NULL = the legacy default stream); calls only enqueue work: they
 *     never allocate, free, synchronise or throw, so a caller may capture them into a hipGraph;
 *   - return value: TIPK_OK, TIPK_EINVAL / TIPK_EUNSUPPORTED for bad arguments, or
 *     -(1000 + hipError_t) when a HIP runtime call failed; `tipk_strerror` names it;
 *   - workspaces (`partial`, slabs) are supplied by the caller; the library borrows pointers for the
 *     duration of the call only;
 *   - thread safety: the launch entry points are re-entrant per (device, stream); one process per GPU for multi-GPU jobs.
 *     Two pieces of state are PROCESS-WIDE (plain globals, read at launch time, no locking): the options of section 0
 *     (`tipk_set_option`) and the flag-wait budget of section 8 (`tipk_peer_set_timeout_ms`) -- set them before launching
 *     from other threads; every exchange of the process shares the one budget.
 */
#ifndef TIPK_H
#define TIPK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TIPK_ABI_VERSION 30

#define TIPK_OK            0
#define TIPK_EINVAL      (-1)
#define TIPK_EUNSUPPORTED (-2)
#define TIPK_EHIP_BASE   (-1000)      /* status = TIPK_EHIP_BASE - hipError_t */

typedef void* tipk_stream_t;          /* hipStream_t */

int         tipk_abi_version(void);
const char* tipk_strerror(int status);
/* digest (16 hex digits) of the sources the library was compiled from; "+debug" appended in
 * -DTIPK_DEBUG builds.  tip_amd/_lib.py refuses a library whose digest differs from the sources
 * next to it (a stale prebuilt .so would silently run old kernels). */
const char* tipk_build_id(void);
/* 0. Host-side options (process-wide; set before launching, never read from the environment):
 *      "gemm_no_stream"      1 = every product through the LDS-tiled kernel (cross-check in tests)
 *      "gemm_thin_k_narrow"  1 = dword body of the Y = att.XB streaming kernel
 *      "gemm_stream_kk"      1 = lane-per-row streaming body for d att
 *      "rg_occupancy"        workgroups per CU tipk_rel_gather aims for: 1, 2 (0 = library default)
 *      "dm_task_kernel"      1 = fused objective through the k/4-lanes-per-position task kernel (the round-2 kernel; A/B runs)
 *      "screen_search"       1 = tipk_distmult_screen filters known pairs by binary search even where the LDS bitmap fits
 *                            (section 4c; both routes return the same bits)
 *      "pair_topk_stream"    1 = tipk_distmult_pair_topk streams rel_w through LDS in tiles even where all of it fits
 *                            (section 4d; both routes return the same bits)
 *      "regimen_global"      1 = tipk_distmult_regimen_topk reads rel_w rows from global memory even where the LDS image
 *                            fits (section 4e; both routes return the same bits)
 *      "pair_rank_stream"    1 = tipk_distmult_pair_rank reads rel_w rows from global memory even where the LDS image fits
 *                            (section 4f; both routes return the same bits)
 *      "partner_rank_global" 1 = tipk_distmult_partner_rank reads z rows from global memory even where the LDS image fits
 *                            (section 4g; both routes return the same bits)
 *      "addon_global"        1 = tipk_distmult_addon_burden reads rel_w rows from global memory even where the LDS image
 *                            fits (section 4i; both routes return the same bits)
 *      "attribution_global"  1 = tipk_rgcn_attribution keeps the per-query table in the caller's workspace even where it fits
 *                            in LDS (section 4j; both routes return the same bits)
 *      "partner_sum_global"  1 = tipk_distmult_partner_sum reads z rows from global memory even where the LDS image fits
 *                            (section 4l; both routes return the same bits)
 *      "combo_no_prefix"     1 = the combination-burden kernel sums every level of every combination; 0: it keeps the sum of
 *                            the slower slots in LDS while the last slot advances (section 4n; both routes return the same
 *                            bits)
 *      "combo_run"           combinations a wavefront of the combination-burden kernel takes in one run, 1..64 (0 = chosen
 *                            from the size of the call; section 4n; every value returns the same bits)
 *      "rg_debug", "dp_debug", "dm_debug"  bit masks that SKIP parts of tipk_rel_gather / tipk_rgcn_dy_products / the decoder kernels
 *                            (timing decompositions): accepted by -DTIPK_DEBUG builds only; a release
 *                            library returns TIPK_EUNSUPPORTED for a non-zero value and its kernels
 *                            contain no skip code.
 *    Unknown name: TIPK_EINVAL. */
int         tipk_set_option(const char* name, int value);
int         tipk_get_option(const char* name, int* value);
/* host query: fills whatever is non-NULL; returns TIPK_OK or a HIP error (e.g. no device). */
int         tipk_device_info(int device, int* n_cu, int* lds_bytes_per_cu, int* wavefront, char* arch, int arch_len);

/* --------------------------------------------------------------------------------------------
 * 1. Segmented gather-sum -- the one sparse-aggregation kernel of the path.
 *
 *      out[row(w)] (or partial[slot(w)]) = sum_{e in [begin_w, end_w)} edge_w[e] * table[row_id[e]]
 *
 * replaces PyG `MessagePassing.propagate` = `index_select` + `torch_scatter.scatter` at
 *   GCNConv            src/layers.py:392,394   (K1: P-P aggregation, edge_w = gcn norm)
 *   MyHierarchyConv    src/layers.py:229-233   (K2: P->D mean)
 *   MyRGCNConv2/Conv   src/layers.py:159-180 / :78-86  (K5/K6: D-D aggregation over Y = att.XB)
 * and their autograd backward (the transposed plan).
 *
 * A *plan* (built once per static graph by tip_amd/plan.py) sorts the edges by output row and cuts
 * every row's edge list into work items of at most `chunk` edges:
 *   items[w] = { begin, end, target, flags }     int32 x 4, items ordered by decreasing length
 *     flags bit0 = 1: the row has one item; `target` is the output row and the epilogue
 *                     (row_scale, bias, relu) is applied here;
 *     flags = 0:      the row is split; `target` is a slot of `partial` ([n_slots x d], dense);
 *                     `tipk_gather_sum_finalize` adds the row's slots in order (deterministic).
 *   Plans built with group_slots = G > 0 never use `partial`: the pieces of a split row occupy
 *   consecutive items inside one aligned block of G items, padded with null items, and are added
 *   in item order through LDS by the kernel itself:
 *     flags bit1 (2): piece; flags bit2 (4): first piece of its row, (flags >> 8) pieces in all,
 *                     `target` = output row, epilogue applied; flags bit3 (8): null item.
 *   One workgroup runs one block: G * lanes-per-item threads (lanes per item = next pow2 of d/4,
 *   or of d when d % 4 != 0) must be a multiple of 64 and <= 1024 (G = 128: d <= 32).
 * d = floats per row (d % 4 == 0: 4..256, or any d <= 64); ld_* = row strides in floats
 * (multiples of 4 when d % 4 == 0; table/out/partial 16-byte aligned in that case).
 * n_table = rows of `table`: below 4 GB a gathered row is addressed as table base + 32-bit byte offset
 * (one multiply per row instead of a 64-bit multiply-add); 0 = unknown (general path).
 *
 * Contracts pinned by tests/test_gpu_gather_paths.py (bit for bit against fp64 on exactly representable sums):
 *   - EVERY output row of the plan is written, rows without edges included: they hold the epilogue of a zero
 *     sum (relu?(bias), or +0).  Nothing outside columns [0, d) of a row is touched (ld_out > d is a column slice).
 *   - E = 0: the plan is one empty item per output row and the launch writes those rows; `row_id` must still be
 *     a non-NULL device address (it is never read) -- n_items > 0 with a NULL table or row_id is TIPK_EINVAL.
 *     tip_amd.ops passes the item list's address for it.  tipk_gather_rows_csr accepts row_id = NULL for E = 0.
 *   - Non-finite table values are added as IEEE values (unweighted sums): +-inf / NaN of a table row reach
 *     exactly the output rows that gather that row (+inf and -inf in one row: NaN) and no other row; lanes
 *     and slots without an edge load nothing.
 *   - The 2^32 switch: n_table * ld_table * 4 < 2^32 takes 32-bit UNSIGNED byte offsets (valid up to the last
 *     row below 4 GiB), anything else (or n_table = 0) 64-bit row addresses -- same results.  tipk_gather_sum
 *     and tipk_gather_sum_finalize serve both; tipk_gather_sum_riders with colsum, tipk_gather_sum_lin and
 *     tipk_gather_rows_csr exist with 32-bit offsets only and return TIPK_EUNSUPPORTED from 2^32 bytes on.
 *   - A table, bias, out or partial that is not 16-byte aligned (or a row stride that is no multiple of 4) takes
 *     the scalar kernels: d <= 64, and a grouped plan must be built for THEIR lane count (next pow2 of d);
 *     wider rows are TIPK_EUNSUPPORTED and nothing is written.
 *   - Two launches on the same inputs give the same bits (fixed summation order, no atomics).
 */
int tipk_gather_sum(const float* table, int64_t ld_table, int64_t n_table /* rows of table (0 = unknown) */,
                    const int32_t* row_id, const float* edge_w /* nullable */,
                    const int32_t* items, int64_t n_items,
                    float* out, int64_t ld_out,
                    float* partial /* nullable when no item is split */,
                    const float* row_scale /* nullable, per out row */,
                    const float* bias /* nullable, [d] */, int relu,
                    int d, int group_slots /* G of the plan, 0 = none */, tipk_stream_t stream);

/* rows[m] = { out_row, first_slot, end_slot } int32 x 3: out[out_row] = epi(sum partial[slots]).
 * max_slots: largest slot count of any row (host knows it from the plan; 0 = unknown) -- picks
 * a slot-per-row kernel for lightly split rows, a workgroup-per-row kernel otherwise. */
int tipk_gather_sum_finalize(const float* partial, const int32_t* rows, int64_t n_rows,
                             float* out, int64_t ld_out,
                             const float* row_scale, const float* bias, int relu,
                             int d, int max_slots, tipk_stream_t stream);

/* tipk_gather_sum on a GROUPED plan whose workgroups have 1024 threads (group_slots x lanes per item; `_supported`), with up
 * to 3 ordered slab sums (section 2: tipk_sum_slabs_group) that are READY at the same point riding in the launch as further
 * workgroups -- the bias-gradient partials of GCNConv 1 next to its transposed aggregation, the split-K slabs of conv2's
 * d W / d bias next to its transposed aggregation (src/layers.py:392-394 under autograd): a dependent 4-us launch less each.
 * Two optional extensions of the epilogue, for the transposed aggregation whose rows are gradients of a ReLU layer's output:
 *   gate [n_out x d] (row stride ld_gate):  out[row] = gate[row] > 0 ? value : 0  (the ReLU backward, src/layers.py:393);
 *   colsum [workgroups x d] (workgroups = ceil(n_items / group_slots), d % 4 == 0): column sums of the finished rows of every
 *   workgroup, in slot order -- the bias gradient's partial rows, added in order by a slab sum (riding in the NEXT gather). */
struct tipk_slab_sum_desc;                         /* section 2 */
int tipk_gather_sum_riders_supported(int d, int group_slots);
int tipk_gather_sum_riders(const float* table, int64_t ld_table, int64_t n_table, const int32_t* row_id, const float* edge_w,
                           const int32_t* items, int64_t n_items, float* out, int64_t ld_out, const float* row_scale,
                           const float* bias, int relu, int d, int group_slots,
                           const float* gate /* nullable */, int64_t ld_gate, float* colsum /* nullable */,
                           const struct tipk_slab_sum_desc* sums /* host, [n_sums <= 3] */, int32_t n_sums,
                           tipk_stream_t stream);

/* tipk_gather_sum on a GROUPED plan with a linear map of every finished row in the same launch:
 *     out[row]  = row_scale[row] * sum (as tipk_gather_sum, no bias / ReLU)          [n_out x d]
 *     out2[row] = relu2?( out[row] . w^T + bias2 )                                     [n_out x d2],  w element (o, i) at w[o w_so + i w_si]
 * Aggregate-then-transform of a GCN layer whose output is needed for FEW rows (conv2 of the P-P encoder: 3 640 of 19 081
 * proteins are read by the P->D stage): A_hat (x W^T) = (A_hat x) W^T, so the dense map runs on the rows that are kept
 * (src/layers.py:392-394 with the rows nobody reads left out), and the layer's forward pass is ONE launch.
 * d in {16, 32, 64} (L = d / 4 lanes hold a row), d2 in {L, 2 L, 4 L} and <= 16, group_slots > 0 (`tipk_gather_sum_lin_supported`). */
int tipk_gather_sum_lin_supported(int d, int d2, int group_slots);
int tipk_gather_sum_lin(const float* table, int64_t ld_table, int64_t n_table, const int32_t* row_id, const float* edge_w,
                        const int32_t* items, int64_t n_items, float* out, int64_t ld_out, const float* row_scale,
                        const float* w, int64_t w_so, int64_t w_si, const float* bias2 /* nullable */, int relu2,
                        float* out2, int64_t ld_out2, int d, int d2, int group_slots, tipk_stream_t stream);

/* Host query, launches nothing: how many workgroups of the GROUPED gather kernel a plan of width d (d % 4 == 0, table below
 * 4 GB) takes are resident on one CU (hipOccupancyMaxActiveBlocksPerMultiprocessor of that kernel instance with the launch's
 * own block size and dynamic LDS).  `map`: 0 = tipk_gather_sum / tipk_gather_sum_riders without colsum, -1 = tipk_gather_sum_riders
 * with colsum, d2 > 0 = tipk_gather_sum_lin with d2 outputs (`tipk_gather_sum_lin_supported`).  The 1024-thread workgroups of
 * the encoder step (d = 16, 32) are built to be resident twice: tip_amd/plan.py sizes their plans for 32 waves per CU.
 * TIPK_EUNSUPPORTED for a (d, group_slots, map) no grouped launch takes. */
int tipk_gather_sum_occupancy(int d, int group_slots, int weighted, int map, int* workgroups_per_cu);

/* --------------------------------------------------------------------------------------------
 * 1c. CSR rows -- the TRANSPOSED D-D pass of a large graph (autograd backward of K5/K6,
 *     src/layers.py:159-180): out[r] = sum_{e in [row_ptr[r], row_ptr[r+1])} table[row_id[e]] for every one
 *     of the n_out rows (all written, also empty ones), where rows are short (config 5: R*N = 20 M rows
 *     (relation, source), 2.5 edges each, table = g' [N x d] cache-resident).  A slot takes 8
 *     consecutive rows: one coalesced pointer load, contiguous ids, 8 gathered rows in flight, one
 *     contiguous output stream -- no work-item descriptors.  Edges sorted by output row (stable);
 *     row_ptr int32 [n_out + 1]; d % 4 == 0, 8 <= d <= 256. */
int tipk_gather_rows_csr(const float* table, int64_t ld_table, int64_t n_table /* rows; table < 4 GB */,
                         const int32_t* row_ptr, const int32_t* row_id,
                         int64_t n_out, float* out, int64_t ld_out, int d, tipk_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * 1b. Relation-local gather -- the D-D aggregation (K5/K6, src/layers.py:159-180) when one
 *     relation's node table fits in LDS (BioSNAP: 645 drugs x 32 floats).  Same sums as
 *     `tipk_gather_sum` over the plan of the same graph, with every gathered row read from LDS:
 *
 *       backward = 0:  table = Y [n_rel * n_nodes, d];  out = partial [n_wg, n_nodes, d] with
 *                      sum_wg partial[wg, o] = sum_r sum_{e in r: out(e)=o} Y[r * n_nodes + tab(e)]
 *                      (combine with tipk_sum_slabs);
 *       backward = 1:  table = g' [n_nodes, d];  out = dY [n_rel * n_nodes, d],
 *                      dY[r * n_nodes + o] = sum_{e in r: out(e)=o} g'[tab(e)]   (every row written).
 *
 *     d: power of two >= 4; n_nodes <= 65535; the columns are cut into blocks until a block's table
 *     (+ accumulators when backward = 0) fits in 158 KB of LDS -- `tipk_rel_gather_supported`.
 *
 *     Relation-local plan (tip_amd/plan.py `build_rel_plan`), all device arrays.  The plan is a
 *     list of n_units WORK UNITS: a unit is one relation, or -- for relations much larger than the
 *     per-workgroup average, which would otherwise set the length of the launch -- every k-th output
 *     position of one relation:
 *       node_at[n_units][n_nodes] uint16: output node at position p of the unit; positions are
 *                               ordered by decreasing run length
 *       runs[n_units][n_nodes][2] (begin relative to the unit's first id, padded length) per position
 *       idx[..]                 uint16 table node of each edge TIMES idx_unit (16-byte aligned array;
 *                               idx_unit = 1, or a power of two up to the bytes of one column-block
 *                               row with n_nodes * idx_unit <= 65535: then a row's LDS address is
 *                               base + idx with no multiply); inside a unit the edges are sorted by
 *                               the position of their OUTPUT node; runs are padded to multiples of 8
 *                               ids with the sentinel n_nodes * idx_unit, whose table row is zero.
 *                               The order of the ids INSIDE a run is free (it only fixes the order of
 *                               the fp32 sum): tip_amd/plan.py orders them so that the slots of one
 *                               ds_read_b128 lane group read different bank quarters (table rows are
 *                               unpadded: node mod (256 / row bytes) is the quarter)
 *       unit_meta[n_units][8]   int32 descriptors, listed in the order the workgroups process them:
 *                               { unit (row of node_at / runs), relation (selects the Y_r block / the
 *                               dY rows), n_pos (positions to walk: backward all of the unit's, so
 *                               every dY row is written exactly once; forward those with edges),
 *                               n_ids (padded), idx offset low, idx offset high (multiple of 8), 0, 0 }
 *       wg_unit_ptr[n_wg+1]     range of unit_meta handled by each of the n_wg workgroups
 *                               (longest-processing-time deal; n_wg = number of CUs)
 */
/* host predicate: number of column blocks the launch will use (grid = n_wg x blocks), 0 = the
 * shape is not supported (use tipk_gather_sum).  row_scale (backward only, nullable): the table
 * rows are multiplied by row_scale[node] while they are staged (g' = g / deg fused). */
int tipk_rel_gather_supported(int64_t n_nodes, int d, int backward);
/* workgroups per CU (1 or 2) the launch of this shape reaches: with 2 the columns are cut finer so that
 * two 1024-thread workgroups share a CU (8 waves per SIMD hide the kernel's LDS round trips); the host
 * builds the plan for  occupancy * CUs / column-blocks  workgroups.  Option "rg_occupancy" (1 | 2). */
int tipk_rel_gather_occupancy(int64_t n_nodes, int d, int backward);
/* ids staged into LDS per pass for this shape (8192 or 16384): a forward work unit with more ids than
 * this reloads its id chunk synchronously, so the host cuts forward units at this size. */
int tipk_rel_gather_chunk(int64_t n_nodes, int d, int backward);
int tipk_rel_gather(int backward, const float* table, int64_t ld_table, int64_t n_nodes, int d,
                    int64_t n_wg, const int32_t* wg_unit_ptr, const int32_t* unit_meta,
                    const uint16_t* idx, int idx_unit, const int32_t* runs, const uint16_t* node_at,
                    const float* row_scale, float* out, int64_t ld_out, tipk_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * 1d. Wave-stream gather:   out[row] = sum_{e: row(e) = row} table[tab(e)]   for a table [n_table x d] that fits in LDS
 *     (one column block of it: `tipk_stream_gather_supported`).  After the table is staged (one barrier) every
 *     wavefront streams through its own list of fixed-size records and never meets the others
 *     (tip_amd/csrc/tipk_rel_stream.hip explains why).  Two uses on the TIP path:
 *       - the TRANSPOSED D-D pass (autograd of src/layers.py:159-180): table = g' [nodes x out], row = relation *
 *         nodes + source node -- the sums of tipk_rel_gather(backward = 1), without its work units;
 *       - the FORWARD D-D pass (src/layers.py:159-180) in pair form: table = att [relations x bases], row =
 *         destination * nodes + source: cell (v, u) = sum of att[r, :] over the relations r that link u -> v
 *         (a drug pair of BioSNAP is linked by 66 relations on average), followed by ONE dense product with
 *         X . basis (tip_amd/ops.py `_RGCN.forward`): Y = att . XB is never formed.
 *       - (round 3) the GCN layers of the P-P graph, both passes (GCNConv.forward via PPEncoder, src/layers.py:392-394):
 *         D^-1/2 (A + I) D^-1/2 X = a row scaling on either side of the plain sum, i.e. row_scale = out_scale =
 *         deg^-1/2, with bias and ReLU in the epilogue.  19 081 proteins fit as 2-column blocks of 8-byte rows
 *         (max_split = 16): the rows come out of LDS instead of through the L2 gather path of tipk_gather_sum.
 *     A lane holds 4 columns (2 when the column block is 2 wide); L = (d / column blocks) / 4 lanes (or 1) form a slot, S = 64 / L slots a wavefront, P = tipk_stream_gather_piece()
 *     steps of 8 ids a cell.  Plan (tip_amd/plan.py `build_stream_plan_rows`), all device arrays:
 *       wave_ptr[n_wg * 16 + 1]  int32: range of bands of every wavefront (wavefront = workgroup * 16 + wave)
 *       cells[n_bands][S]        uint32: row (24 bits) | steps << 24 (0 .. P) | first << 28 | last << 29 | log2 k << 30.
 *                                A slot adds the steps' rows to a register sum that is cleared on `first` and
 *                                written to out[row] on `last`: a run longer than P steps continues in the SAME
 *                                slot of the wavefront's next band; 0 = idle cell.  log2 k > 0 (on the last band
 *                                of a WIDE run, in all its slots): the run was cut into k = 2, 4 or 8 sub-runs in
 *                                adjacent slots s0 .. s0 + k - 1 (s0 a multiple of k); their sums are added in
 *                                the fixed order  s <- s + 2^j,  j = 0, 1, ..,  and slot s0 (the one with `last`)
 *                                writes the row -- a slot's run is a chain of dependent steps, and the longest
 *                                run of the graph would otherwise set the length of the launch
 *       ids[n_bands][P][S][8]    uint16: table row * idx_unit of the edges (see 1b), runs padded to 8 with the
 *                                sentinel n_table * idx_unit (a zero row); steps beyond a cell's count are not read
 *       zero_ptr[n_wg * 16 + 1], zero_rows[]  int32: the rows without edges, dealt to the wavefronts; zero_ptr
 *                                = NULL: those rows are left untouched (the consumer masks them -- section 2b
 *                                row_used -- or they live in a buffer that was zeroed once)
 *     rows < 2^24.  row_scale (nullable): row_scale[i] * table[i] is what is staged.
 *     Epilogue of a finished row (rows without edges included): relu?(out_scale[row] * sum + bias[col]); out_scale /
 *     bias nullable.  max_split: the largest number of column blocks the caller accepts (every block walks all the ids
 *     again): 4 on the D-D passes, 16 for the P-P graph (which also admits 2-column blocks).
 *     STREAMED OUTPUT: the launches whose rows are write-once pair-form output -- tipk_stream_gather with kind = 1 (pair
 *     cells), tipk_stream_gather_two, and tipk_stream_gather_parts / _parts_two of section 2e -- write every row (zero rows
 *     included) with 16-byte stores that do not keep the line in the writing XCD's L2, where a lane group covers whole
 *     128-byte lines (column blocks of 32 columns and more).  Same values, same rows; but a kernel that re-reads those rows
 *     right behind the launch finds none of them L2-resident -- they come from the Infinity Cache / HBM.
 */
/* column blocks of the launch (grid = n_wg x blocks); 0 = the table does not fit in LDS */
int tipk_stream_gather_supported(int64_t n_table, int d, int max_split);
/* two tables of the same shape on ONE plan in one launch (no zero rows, no scaling, no epilogue): out0 <- table0, out1 <- table1;
 * the pair cells of both R-GCN layers of an encoder (they share the graph; the cells depend on the parameters only).  One column
 * block only (tipk_stream_gather_supported(n_table, d, 1) == 1), d in {16, 32, 64}.  out0 / out1 bypass L2 residency for d >= 32
 * (STREAMED OUTPUT above). */
int tipk_stream_gather_two(const float* table0, const float* table1, int64_t ld_table, int64_t n_table, int d, int64_t n_wg,
                           const int32_t* wave_ptr, const uint32_t* cells, const uint16_t* ids, int idx_unit,
                           float* out0, float* out1, int64_t ld_out, tipk_stream_t stream);
int tipk_stream_gather_piece(void);
int tipk_stream_gather(const float* table, int64_t ld_table, int64_t n_table, int d, int64_t n_wg,
                        const int32_t* wave_ptr, const uint32_t* cells, const uint16_t* ids, int idx_unit,
                        const int32_t* zero_ptr, const int32_t* zero_rows, const float* row_scale,
                        float* out, int64_t ld_out, int kind /* 0 | 1: names the kernel instance in profiles; 1 (pair cells): `out` bypasses L2 residency (STREAMED OUTPUT above) */,
                        int max_split, const float* out_scale, const float* bias, int relu, tipk_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * 2. Dense fp32 GEMM on the matrix cores (v_mfma_f32_32x32x2_f32: exact fp32 fma chain).
 *
 *   C[z] = relu?( alpha * sum_{q<kbatch} A[z,q] (m x k) . B[z,q] (k x n) + C_in[z] ),  z < batch
 *
 * With ksplit > 1 the k range is cut into `ksplit` slabs: slab s holds the partial product over
 * its k range at c + s*c_ss (c_in/relu must be unset); `tipk_sum_slabs` combines them in order.
 *
 * replaces the `torch.matmul`/`mm` calls of the path:
 *   W = att @ basis.view(B,-1), x_j[s:e] @ w[et], x @ root   src/layers.py:163-172,184  (K4,K5,K7)
 *   aggr_out[n_src:] @ weight                                 src/layers.py:239          (K2)
 *   GCNConv.lin                                               src/layers.py:392,394      (K1)
 * and their backward products.  Element (i,j) of A[z,q] is a[z*a_sz + q*a_sq + i*a_sm + j*a_sk]
 * (strides in floats, so transposes and the basis-decomposition reshapes need no copies).
 *
 * k == 0 is an empty sum: C[z] = relu?(C_in[z]), or zeros without c_in (every slab of a split product: zeros); a and b are
 * not read and may be NULL.  m == 0, n == 0 or batch == 0: nothing is written.
 */
typedef struct tipk_gemm_desc {
    int64_t m, n, k;
    int64_t batch, kbatch;
    int64_t ksplit;                                /* >= 1: split K into this many slabs */
    const float* a; int64_t a_sm, a_sk, a_sq, a_sz;
    const float* b; int64_t b_sk, b_sn, b_sq, b_sz;
    float*       c; int64_t c_sm, c_sz, c_ss;      /* C row-major (column stride 1); c_ss = slab stride */
    const float* c_in; int64_t cin_sm, cin_sz;     /* nullable; may alias c */
    float alpha;
    int   relu;
} tipk_gemm_desc;

int tipk_gemm_f32(const tipk_gemm_desc* desc /* host */, tipk_stream_t stream);

/* Which kernel body tipk_gemm_f32 runs for `desc` (grouped != 0: tipk_gemm_f32_group, for `desc` as a member), under the
 * current "gemm_no_stream" / "gemm_thin_k_narrow" / "gemm_stream_kk" options.  A pure host function -- a, b, c and c_in are
 * looked at as addresses only (NULL, alignment), nothing is launched -- and THE decision both entry points dispatch on.
 * Returns the negative status tipk_gemm_f32 would return, else  body | flags:
 *   body  (code & TIPK_ROUTE_BODY_MASK)
 *     TIPK_ROUTE_NONE            nothing to compute (m, n or batch == 0)
 *     TIPK_ROUTE_TILED_128X32    LDS-tiled, 4 x 1 waves of 32 x 32   (n <= 32)
 *     TIPK_ROUTE_TILED_32X128    LDS-tiled, 1 x 4 waves              (m <= 32 < n)
 *     TIPK_ROUTE_TILED_64X64     LDS-tiled, 2 x 2 waves
 *     TIPK_ROUTE_TILED_128X128   LDS-tiled, 2 x 2 waves of 2 x 2 accumulators (m, n >= 512, ksplit == 1; never grouped: 64 x 64)
 *     TIPK_ROUTE_THIN_K          streaming, k <= 32, dword accesses  (never grouped: tiled)
 *     TIPK_ROUTE_THIN_K4         streaming, k <= 32, 16-byte accesses (n % 4 == 0, aligned rows; never grouped: tiled)
 *     TIPK_ROUTE_THIN_M          streaming, m <= 32, long k
 *     TIPK_ROUTE_KK              streaming, n <= 32, both operands contiguous in k ("gemm_stream_kk" only)
 *   flags, tiled bodies only
 *     TIPK_ROUTE_TWO_BUFFERS     two LDS buffers (unset: one -- a K range of a single 32-term tile, and every 128 x 128 product;
 *                                grouped members always run with two)
 *     TIPK_ROUTE_A_KFAST         consecutive threads of the A tile loader walk k (a_sk == 1 or a_sm != 1), else rows
 *     TIPK_ROUTE_B_KFAST         the same for B (b_sk == 1 and b_sn != 1)
 * The streaming bodies are chosen for products of >= 2^20 elements in m*n, n*k or m*k with kbatch == 1 and k >= 1
 * (tip_amd/csrc/tipk_gemm.hip: stream_kind).  The narrow thin-k body, thin_m and every tiled body add the terms of one element in
 * the same order: their results are bit-identical to each other; thin_k4 and kk pair k differently.  Non-finite inputs
 * included: no body multiplies a term outside its k range (the streaming bodies clear BOTH operands of the lanes past the end
 * of k), so an infinity in the last row of B gives the infinities of the fp64 product on every route. */
#define TIPK_ROUTE_NONE 0
#define TIPK_ROUTE_TILED_128X32 1
#define TIPK_ROUTE_TILED_32X128 2
#define TIPK_ROUTE_TILED_64X64 3
#define TIPK_ROUTE_TILED_128X128 4
#define TIPK_ROUTE_THIN_K 5
#define TIPK_ROUTE_THIN_K4 6
#define TIPK_ROUTE_THIN_M 7
#define TIPK_ROUTE_KK 8
#define TIPK_ROUTE_BODY_MASK 15
#define TIPK_ROUTE_TWO_BUFFERS 16
#define TIPK_ROUTE_A_KFAST 32
#define TIPK_ROUTE_B_KFAST 64
int tipk_gemm_route(const tipk_gemm_desc* desc /* host */, int grouped);

/* Up to TIPK_GROUP_MAX independent products in ONE launch (no ordering between them; outputs must
 * not overlap any input of the group).  Each product is computed exactly as tipk_gemm_f32 would
 * (same k order -> bit-identical; tipk_gemm_route(desc, 1) names the body: a product tipk_gemm_f32 would stream through the
 * thin-k bodies runs LDS-tiled here -- the bits of the narrow thin-k body, not of thin_k4 -- and 128 x 128 tiles become
 * 64 x 64).  Used where the path needs several small
 * products at the same point of the dependent chain: XB and X root going forward
 * (src/layers.py:163-172 and :184), d basis / d root / both halves of dX going back. */
#define TIPK_GROUP_MAX 6
int tipk_gemm_f32_group(const tipk_gemm_desc* descs /* host, [count] */, int32_t count, tipk_stream_t stream);

/* out[i] = alpha * sum_{s<n_slabs} in[s*slab_stride + i] (+ out[i] if accumulate), i < count.
 * Ordered (deterministic) reduction of split-K slabs / per-workgroup partials. */
int tipk_sum_slabs(const float* in, int64_t n_slabs, int64_t slab_stride, int64_t count,
                   float alpha, int accumulate, float* out, tipk_stream_t stream);
/* same with a fused epilogue: out[i] = relu?( alpha * row_scale[i / cols] * sum_s in[s][i] + addend[i]
 * (+ out[i]) ); row_scale / addend nullable.  Finishes an R-GCN layer in one pass:
 * relu( D^-1 sum_partials + X root )  (src/layers.py:184, :547). */
int tipk_sum_slabs_ex(const float* in, int64_t n_slabs, int64_t slab_stride, int64_t count,
                      float alpha, int accumulate, const float* row_scale, int64_t cols,
                      const float* addend, int relu, float* out, tipk_stream_t stream);
/* the same for up to TIPK_GROUP_MAX independent slab sets in one launch (arguments as above);
 * gate (nullable, [count]): out[i] = gate[i] > 0 ? value : 0 -- the ReLU backward of the layer that
 * produced the gradient's input (src/layers.py:547), applied while the gradient is finished. */
typedef struct tipk_slab_sum_desc {
    const float* in; int64_t n_slabs, slab_stride, count;
    float alpha; int accumulate;
    const float* row_scale; int64_t cols;
    const float* addend; int relu;
    const float* gate;
    float* out;
} tipk_slab_sum_desc;
int tipk_sum_slabs_group(const tipk_slab_sum_desc* descs /* host, [count] */, int32_t count, tipk_stream_t stream);

/* Products whose reduction is split over the 16 waves of ONE workgroup, plus ordered slab sums that are ready at
 * the same point, in ONE launch.  The backward pass of an R-GCN layer (autograd of src/layers.py:159-184) ends in
 * d basis[b] = X^T dXB[b], d root = X^T g and dX = sum_b dXB[b] basis[b]^T + g root^T: few output tiles, reductions of
 * 645 .. 1 056 terms.  A workgroup owns a 32 x 32 output tile, deals its K tiles (32 terms; the kbatch terms of p and the
 * optional second product a2 . b2 are further tiles) to its waves in contiguous runs and adds the partial tiles in
 * wave order (deterministic) -- no slabs, no second launch.
 *   p:     as tipk_gemm_f32 (batch, kbatch, strides, c_in, alpha, relu); ksplit must be 1
 *   a2/b2: nullable second product [m x k2] . [k2 x n] added to the same output (batch must be 1)
 *   gate:  nullable, laid out like the output: out = gate > 0 ? value : 0
 * Shapes: at most 64 K tiles in all (2 048 terms), at most 4096 output tiles (TIPK_EUNSUPPORTED otherwise: tipk_gemm_f32_group). */
typedef struct tipk_wg_gemm_desc {
    tipk_gemm_desc p;
    const float* a2; int64_t a2_sm, a2_sk;
    const float* b2; int64_t b2_sk, b2_sn;
    int64_t k2;
    const float* gate; int64_t gate_sm, gate_sz;
} tipk_wg_gemm_desc;
#define TIPK_WG_GEMM_MAX 4
#define TIPK_WG_SUMS_MAX 3
int tipk_gemm_wg_group_supported(const tipk_wg_gemm_desc* desc /* host */);
int tipk_gemm_wg_group(const tipk_wg_gemm_desc* descs /* host, [count <= TIPK_WG_GEMM_MAX] */, int32_t count,
                       const tipk_slab_sum_desc* sums /* host, [n_sums <= TIPK_WG_SUMS_MAX], nullable */, int32_t n_sums,
                       tipk_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * 2c. The dense half of the pair-form D-D forward pass (src/layers.py:159-180; tip_amd/ops.py `_RGCN.forward`):
 *
 *        slabs[g][v, c] = sum_{u in group g} sum_b cells[u][v][b] * xb[u][b][c]        g < n_src / group
 *
 *     cells [n_src][n_dst][n_bases] = the pair cells written by tipk_stream_gather (table = att), xb
 *     [n_src][n_bases][32] = X . basis per source node, rows PADDED to 32 columns with zeros beyond d; n_src is the node count rounded up to a multiple of
 *     `group` with blocks that stay zero.  slabs [n_src / group][n_dst][d] are added in order by
 *     tipk_sum_slabs_ex (which also applies 1 / deg, + X root and the ReLU).  n_bases in {8, 16, 32}, d <= 32
 *     (`tipk_pair_product_supported`; otherwise tipk_gemm_f32 with kbatch = group does the same sums).
 *     symmetric != 0: every relation links u -> v iff it links v -> u (BioSNAP), so cells[u][v] == cells[v][u]
 *     and the gather only built the cells with u <= v (half the edges); cell (u, v) with v < u is read at (v, u).
 *     links (nullable): uint32 [n_src][ceil(n_dst / 32)], bit r of word (u, t) = "pair (u, 32 t + r) is linked" (rows of the
 *     padding nodes zero; on a symmetric graph bit (u, v) == bit (v, u)): the cell of an unlinked pair is not fetched (it is
 *     zero by construction; `zeros` = >= n_bases * 4 bytes of zeros (128 B at n_bases = 32), 16-byte aligned, read in its place).
 *     xbt (nullable, [n_dst][d][n_bases], 16-byte aligned): XB of the first n_dst source nodes written back with the bases
 *     innermost -- the operand layout of the backward pass (tipk_rgcn_node_products xbt), from the LDS stage of this kernel.
 */
int tipk_pair_product_supported(int n_bases, int d);
int tipk_pair_product(const float* cells, const float* xb, int64_t n_src, int64_t n_dst, int n_bases, int d,
                      int group, int symmetric, const uint32_t* links, const float* zeros, float* xbt /* nullable */,
                      float* slabs, tipk_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * 2b. Both consumers of dY (the gradient of Y = att . XB, src/layers.py:163-172 under autograd) in
 *     one pass over dY [n_rel x n_cols] (n_cols = nodes * out channels; 91 MB at BioSNAP layer 1):
 *
 *        dXB [b, c] = sum_r att[r, b] * dY[r, c]       datt[r, b] = sum_c dY[r, c] * XB[b, c]
 *
 *     Results arrive as slabs to be added in order (tipk_sum_slabs_group):
 *        dxb_slabs  [row_slabs][n_bases x n_cols]   one per range of relations
 *        datt_slabs [col_slabs][n_rel x n_bases]    one per chunk of 512 columns
 *     `tipk_rgcn_dy_products_plan` returns the slab counts (both 0: shape not supported -- n_bases > 32;
 *     use two tipk_gemm_f32 then).  The datt slabs are n_bases / 512 of the size of dY.
 *     row_used (nullable; then n_nodes = n_cols / columns per node): uint32 [ceil(n_rel / 32)][n_nodes], bit
 *     (r & 31) of word (r >> 5, node) = "relation r has an edge leaving node" = row (r, node) of dY holds data.
 *     More than half of the (relation, source) rows of BioSNAP have no edge: with the mask the transposed
 *     gather (section 1d, zero_ptr = NULL) does not write their zeros -- 48 of 91 MB at layer 1 -- and
 *     whatever the buffer holds there is cleared bitwise after it is loaded.
 */
int tipk_rgcn_dy_products_plan(int64_t n_rel, int64_t n_cols, int n_bases, int* col_slabs, int* row_slabs);
int tipk_rgcn_dy_products(const float* dy, int64_t ld_dy, const float* att, int64_t ld_att,
                          const float* xb, int64_t ld_xb, int64_t n_rel, int64_t n_cols, int n_bases,
                          const uint32_t* row_used, int64_t n_nodes,
                          float* dxb_slabs, float* datt_slabs, tipk_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * 2d. The same two products as 2b on the COMPACT, node-major form of dY (autograd of src/layers.py:163-172 and of
 *     the scatter-mean at :159-180, for graphs whose transposed pass runs as tipk_stream_gather):
 *
 *        dXB [b, u, c] = sum_{r leaves u} att[r, b] * dY[(u, r), c]      datt[r, b] = sum_u sum_c dY[(u, r), c] * XB[b, u, c]
 *
 *     dyc [n_rows + 1][d]: one row per (source node u, relation r) pair that has an edge (BioSNAP: 47 % of the
 *       R x N pairs), grouped by node, ascending relation inside a node -- the row numbers are what the plan of the
 *       transposed gather (section 1d) writes into its cells, so the gather produces this layout directly; row
 *       n_rows must hold zeros (pairs without an edge read it).
 *     node_desc [n_nodes][4]  { node u, first row, end row, 0 } of the nodes by DECREASING row count (launch order of
 *       the per-node workgroups; 16-byte aligned);   row_rel [n_rows]  relation of a row;
 *     pos [n_nodes][ceil(n_rel / 64) * 64]  row of (u, r), or n_rows when the pair has no edge / r >= n_rel.
 *     xb element (b, u, c) at xb[b * xb_sb + u * xb_su + c] (strides multiples of 4 floats), dxb likewise: written
 *     COMPLETE (no slabs); datt_slabs [att_slabs][n_rel][n_bases] are added in order by tipk_sum_slabs(_group).
 *     xbt (optional): the same values as [n_nodes][d][n_bases] (contiguous) -- the d att product then reads a column of
 *     all bases as ONE 128-byte line instead of 32 lines (the vector-memory address path bounds that product).
 *     d in {16, 32, 64, 128}, n_bases <= 32 (`tipk_rgcn_node_products_plan` returns att_slabs = 0 otherwise: use the
 *     dense form 2b).  All sums in fixed order: bitwise reproducible.
 */
int tipk_rgcn_node_products_plan(int64_t n_nodes, int d, int64_t n_rel, int n_bases, int* att_slabs);
int tipk_rgcn_node_products(const float* dyc, int64_t n_rows, int d, const int32_t* node_desc, const int32_t* row_rel,
                            const int32_t* pos, int64_t n_nodes, int64_t n_rel,
                            const float* att, int64_t ld_att, int n_bases,
                            const float* xb, int64_t xb_sb, int64_t xb_su, const float* xbt /* nullable */,
                            float* dxb, int64_t dxb_sb, int64_t dxb_su, float* datt_slabs, tipk_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * 2e. The BACKWARD pass of the pair form 2c (autograd of src/layers.py:159-180 for graphs whose forward pass ran as
 *     cells + tipk_pair_product): with g' = g / deg and the cells C the forward pass left in place,
 *
 *        dxb[b, u, c]     = sum_{v linked to u} C[u, v, b] * g'[v, c]
 *        pg [slot(u, v)]  = XB[u] . g'[v]            one row of n_bases floats per LINKED (u, v): d C[u, v, :]
 *        datt[r, :]       = sum over the pairs (u, v) that relation r links of pg[slot(u, v)]
 *
 *     -- no row of dY = A_r^T g' is ever formed (sections 2b / 2d), nothing is per relation until the last line, and on a
 *     symmetric graph that line walks HALF the edges: datt[r] = sum_{u <= v} (pg[slot(u, v)] + pg[slot(v, u)]).
 *     tipk_rgcn_pair_grads (the first two lines), plan arrays of tip_amd/plan.py `build_pair_bwd_plan`:
 *       slots [n_slots][4]  { v, float bits of 1 / deg(v), cell line of (u, v), row of pg }: the neighbours of a node in runs
 *          of 32 (n_slots % 32 == 0; pads carry a valid v / line, the factor 0.0f and a dump row, so they add zeros -- g must
 *          be finite); cell line L = the n_bases floats at cells + L * n_bases (a symmetric forward pass keeps (min, max) only);
 *       node_desc [n_nodes][4]  { node u, its first slot, its tiles of 32 slots, 0 } by DECREASING tile count;
 *       tile_node [n_slots / 32]  the node of every tile (the pair-gradient rows are computed one tile per wavefront);
 *       cells: n_lines lines of n_bases floats; xb [n_nodes][n_bases][32] as in 2c; g [n_nodes][ld_g]; dxb element
 *       (b, u, c) at dxb[b * dxb_sb + u * dxb_su + c], written COMPLETE; pg [pg_rows][n_bases]: the gradient row of a slot
 *       is written to row slots[..][3] -- the place the gather below stages it from, so pg needs no index on the way out.
 *     n_bases = 32, d in {16, 32} (`tipk_rgcn_pair_grads_supported`).  All sums in fixed order: bitwise reproducible.
 *     tipk_stream_gather_parts (the last line) is tipk_stream_gather (1d) with a table PER WORKGROUP: the pairs (sorted) are
 *     cut into partitions of at most part_len consecutive rows that fit in LDS, row i of partition p = table[part_first[p] + i]
 *     + table[second + part_first[p] + i] (table = pg: first half = the rows of (u, v), u <= v, second half = the rows of
 *     their mirrors; rows nobody writes hold zeros), wg_part [n_wg] = the partition a workgroup stages, ids = rows counted
 *     from the partition's first, output rows = p * n_rel + r (out [n_parts * n_rel][d], added over p in order by
 *     tipk_sum_slabs(_group)).  d = 32 (one 128-byte row per pair); every partition is staged part_len rows long.  The plan is
 *     walked with 8 lanes per row (build it for lanes = 8, whatever column split the att table of the forward cells needs).
 *     The slabs `out` (out0 / out1 of tipk_stream_gather_parts_two) bypass L2 residency (1d, STREAMED OUTPUT); pg and dxb of
 *     tipk_rgcn_pair_grads are plain write-back stores.
 */
int tipk_rgcn_pair_grads_supported(int n_bases, int d);
int tipk_rgcn_pair_grads(const float* cells, int64_t n_lines, const float* xb, const float* g, int64_t ld_g,
                         int64_t n_nodes, int n_bases, int d, const int32_t* node_desc, const int32_t* slots,
                         const int32_t* tile_node, int64_t n_slots, float* dxb, int64_t dxb_sb, int64_t dxb_su, float* pg, int64_t pg_rows,
                         tipk_stream_t stream);
int tipk_stream_gather_parts(const float* table, int64_t ld_table, int d, int64_t second, const int32_t* part_first,
                             int64_t part_len, const int32_t* wg_part, int64_t n_wg, const int32_t* wave_ptr,
                             const uint32_t* cells, const uint16_t* ids, int idx_unit, const int32_t* zero_ptr /* nullable */,
                             const int32_t* zero_rows, float* out, int64_t ld_out, tipk_stream_t stream);
/* Round 6: the d att gathers of BOTH R-GCN layers of an encoder in one launch (the layers share the plan): grid.y = 1
 * stages its partitions from table1 and writes out1; everything else as tipk_stream_gather_parts. */
int tipk_stream_gather_parts_two(const float* table0, const float* table1, int64_t ld_table, int d, int64_t second,
                                 const int32_t* part_first, int64_t part_len, const int32_t* wg_part, int64_t n_wg,
                                 const int32_t* wave_ptr, const uint32_t* cells, const uint16_t* ids, int idx_unit,
                                 const int32_t* zero_ptr, const int32_t* zero_rows, float* out0, float* out1,
                                 int64_t ld_out, tipk_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * 2f. Forward aggregation of an R-GCN layer on LARGE node sets without Y = att . XB (src/layers.py:159-180 with
 *     W_r = sum_b att[r, b] basis_b):   agg[v] = sum_b T[b, v, :] basis_b,
 *
 *        T[b, v, i] = sum_{e -> v} att[r_e, b] * x[src_e, i]          one matrix product per DESTINATION, K = its edges
 *
 *     -- 164 MB instead of the 10 GB of Y at config 5 (N = 10 000, R = 2 000, d = 128); the second product is a
 *     batch-reduced tipk_gemm_f32.  edges [E]: uint32 rel | src << bits, grouped by destination (bits = the return value of
 *     `tipk_rgcn_dest_products_supported`, 0 = shape not supported: n_bases > 32, or ids that do not fit 32 bits);
 *     node_desc [n_nodes][4] { node v, its first edge, its edges, 0 } by DECREASING edge count (16-byte aligned);
 *     T element (b, v, i) at t[b * t_sb + v * t_sv + i], every element written.  Sums in edge order per wave, the four
 *     waves of a node in wave order: bitwise reproducible.
 */
int tipk_rgcn_dest_products_supported(int64_t n_nodes, int64_t n_rel, int n_bases, int d_in);
int tipk_rgcn_dest_products(const float* x, int64_t ld_x, int d_in, const float* att, int64_t ld_att, int n_bases,
                            int64_t n_nodes, int64_t n_rel, const int32_t* node_desc, const uint32_t* edges,
                            float* t, int64_t t_sb, int64_t t_sv, tipk_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * 2g. The hand-over between two R-GCN layers in one launch (src/layers.py:545-548): the ordered slab sum that ends a
 *     layer's forward pass (the 16 slab lanes and the order of additions of tipk_sum_slabs_ex, epilogue relu?(row_scale * sum +
 *     addend)) -> x [n_rows][32], and at once the next layer's row-local products: xb [row][n_bases][32] = x basis (node-major,
 *     rows padded to 32 columns: the operand of 2c; columns >= d_out are not written) and xroot [n_rows][d_out] = x root.
 *     slabs [n_slabs][n_rows][32] (slab_stride floats apart); basis [n_bases][32][d_out], root [32][d_out], contiguous.
 *     d_in = 32 only (TIPK_EUNSUPPORTED otherwise: tipk_sum_slabs_ex + tipk_gemm_f32_group do the same).
 */
int tipk_sum_slabs_xb(const float* slabs, int64_t n_slabs, int64_t slab_stride, int64_t n_rows, int d_in,
                      const float* row_scale /* nullable */, const float* addend /* nullable */, int relu, float* x,
                      const float* basis, const float* root, int n_bases, int d_out, float* xb, float* xroot,
                      tipk_stream_t stream);
/* host query, launches nothing: 1024-thread workgroups of the kernel behind tipk_sum_slabs_xb resident on one CU for this
 * d_out (hipOccupancyMaxActiveBlocksPerMultiprocessor; built to be 2, so that a step's workgroups run in one round) */
int tipk_sum_slabs_xb_occupancy(int d_out, int* workgroups_per_cu);

/* --------------------------------------------------------------------------------------------
 * 2h. LARGE node sets, both passes: the (relation, node) row sums are assembled in LDS and multiplied there -- neither
 *     Y = att . XB nor dY = A_r^T g' exists in memory (src/layers.py:159-180 and its autograd):
 *
 *        S[(r, v), :] = sum_{e in (r, v)} table[other_e, :]
 *        t[b, v, :]   = sum_r att[r, b] S[(r, v), :]               forward: table = X, rows by destination (agg = sum_b t_b basis_b);
 *                                                                   backward: table = D^-1 g', rows by source (t = d XB)
 *        d att[r, b]  = sum_v < S[(r, v), :], xb[b, v, :] >         only with xb != NULL: slab s of datt_slabs [n_slabs][n_rel][n_bases]
 *                                                                   holds the partial sum of 8 nodes x 32 channels (sum the slabs)
 *
 *     entries [n_batches][2][16] int32: per (node, tile of 32 relations) batches of 16 words per HALF (half = rel & 1),
 *     a half's list sorted by relation, word = inside << 24 | other << 8 | 4 * (rel % 32) with inside = 0 at the first word
 *     of a (relation, node) row and 1 at its other words, padding word 128 (only at the end of a list); a node's batches are
 *     consecutive, tile after tile; desc [n_nodes][ceil(n_rel / 32)][2] = { first batch, batches >= 1 }; `entries` ends with 8
 *     batches of padding behind the last node's (the load pipeline runs 8 batches ahead of the sums).
 *     channels % 32 == 0, n_bases <= 32, n_nodes <= 65 536 (`_supported`), ld_table % 64 == 0 and < 16 384;
 *     t [n_bases][n_nodes * channels], every element written; n_slabs = `tipk_rgcn_row_products_slabs`.  Sums in entry
 *     order: bitwise reproducible.
 */
int tipk_rgcn_row_products_supported(int64_t n_nodes, int64_t n_rel, int n_bases, int channels);
int64_t tipk_rgcn_row_products_slabs(int64_t n_nodes, int channels);
int tipk_rgcn_row_products(const float* table, int64_t ld_table, int64_t n_nodes, int channels, const float* att,
                           int64_t ld_att, int64_t n_rel, int n_bases, const int32_t* entries, const int32_t* desc,
                           const float* xb /* nullable */, int64_t ld_xb, float* t, float* datt_slabs /* nullable */,
                           tipk_stream_t stream);

/* The same two products with WAVE-UNIFORM entries (channels % 64 == 0; any node count whose table fits 2 GB): a wave =
 * (node, 64 channels), one entry per step for the whole wave, so the entry's table offset, LDS row offset and inside-row flag
 * are scalar operands (1 VALU instruction per entry; the fp32 MFMA and the VALU of a SIMD do not overlap on gfx950).
 * entries [n_batches][2][16] int32: ONE list per (node, tile of 32 relations) sorted by relation and padded to 16 entries,
 * plane 0 = BYTE offset of the gathered table row (other * ld_table * 4), plane 1 = 260 * (rel % 32) | 0x3f800000 at every entry
 * of a (relation, node) row but its first (padding: 0 / 260 * 32); desc, padding batches at the end, t and datt_slabs as above
 * (a slab = 8 nodes x 64 channels). */
int tipk_rgcn_row_products_s_supported(int64_t n_nodes, int64_t n_rel, int n_bases, int channels);
int tipk_rgcn_row_products_s(const float* table, int64_t ld_table, int64_t n_nodes, int channels, const float* att,
                             int64_t ld_att, int64_t n_rel, int n_bases, const int32_t* entries, const int32_t* desc,
                             const float* xb /* nullable */, int64_t ld_xb, float* t, float* datt_slabs /* nullable */,
                             tipk_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * 3. Small row-wise glue (each replaces one or more torch elementwise/copy kernels, K3/K8).
 */
/* out[c, r] = in[r, c]  -- `lin(x)` for identity features is W^T (src/layers.py:392 with
 * prepare.py:22-23), and dW = (dXlin)^T on the way back. */
int tipk_transpose(const float* in, int64_t rows, int64_t cols, float* out, tipk_stream_t stream);

/* out[r, c] (+)= in[r, c] * (row_mul ? row_mul[r] : 1) / (row_div ? row_div[r] : 1)
 *               * (gate ? (gate[r, c] > 0) : 1)
 * covers x/d_norm + cat/add (src/layers.py:534-539), 1/deg scaling of upstream gradients and the
 * ReLU backward gate (src/layers.py:393,547). */
int tipk_rows_affine(const float* in, int64_t ld_in,
                     const float* row_mul, const float* row_div,
                     const float* gate, int64_t ld_gate,
                     float* out, int64_t ld_out,
                     int64_t rows, int64_t cols, int accumulate, tipk_stream_t stream);

/* out[r, c] = in[r, c] * (gate[r, c] > 0)  AND  scratch[g, c] = the column sums of out over the rows
 * of workgroup g (g < tipk_gate_colsum_groups(rows, cols); 0 = unsupported, cols > 256): the ReLU
 * backward of GCNConv 1 (src/layers.py:393) and stage 1 of its bias gradient in one pass; the groups
 * are added in order by tipk_sum_slabs. */
int tipk_gate_colsum_groups(int64_t rows, int64_t cols);
int tipk_gate_colsum(const float* in, int64_t ld_in, const float* gate, int64_t ld_gate,
                     float* out, int64_t ld_out, int64_t rows, int64_t cols, float* scratch,
                     tipk_stream_t stream);

/* The drug feature mix of FMEncoder in one forward launch (src/layers.py:526-539 with the dense map of
 * MyHierarchyConv, :239):   x0 = cat(xd / d_norm, mean W)  (cat != 0)   or   x0 = xd / d_norm + mean W  (q == ne).
 * xd [rows x ne], mean [rows x p], W [p x q] row-major contiguous, p, q <= 64; d_norm nullable (= 1). */
int tipk_drug_mix_fwd(const float* xd, int64_t ld_xd, const float* d_norm, const float* mean, int64_t ld_mean,
                      const float* w, int p, int q, int64_t rows, int ne, int cat, float* out, int64_t ld_out,
                      tipk_stream_t stream);

/* The P -> D stage fused with the drug feature mix, one launch per pass (src/layers.py:526-539 with MyHierarchyConv,
 * :229-242: mean over a drug's protein targets, dense map, /d_norm, cat | add):
 *     mean[d, :] = scale[d] * sum_{e in [ptr[d], ptr[d + 1])} h[src[e], :]         (scale = 1 / max(1, #targets))
 *     out[d, :]  = cat(xd[d] / d_norm[d], mean[d] W)   (cat != 0)   or   xd[d] / d_norm[d] + mean[d] W   (q == ne)
 *   h [n_src x p] (row stride ld_h), W [p x q] contiguous, p and q even and <= 64 (tipk_drug_mix_gather_supported),
 *   CSR by drug: ptr int32 [rows + 1], src int32 [edges]; `mean` [rows x p] contiguous is an OUTPUT (kept for the backward).
 *   wg_desc int32 [n_wg][2] = { first, n | W << 8 } of a 16-wave workgroup: rows order[first .. first + n) (order = NULL: the
 *   drugs first .. first + n - 1 themselves), W wavefronts per row sharing its edges, n <= 16 / W, W in {1, 4, 16} (W = 0: the
 *   round-5 form -- n consecutive drugs a wavefront each, or ONE drug on all 16) -- every drug exactly once.  Round 6 deals the
 *   drugs by edge count (tip_amd.layers.hier_graph): > 512 edges alone, 65 ... 512 four to a workgroup, the rest sixteen.
 * Backward, from g = d out [rows x (cat ? ne + q : ne)], one launch (tipk_drug_mix_bwd):
 *     g_xd   = g[:, :ne] / d_norm                          (nullable: not wanted)
 *     g_mean = g_pd W^T                                    [rows x p] contiguous (nullable), g_pd = the last q (cat) / all
 *                                                          (add) columns of g; the caller gathers it back to the source rows
 *                                                          on the transposed plan (tipk_gather_sum, edge weights = scale)
 *     g_w    = mean^T g_pd                                 [p x q]
 * All sums in fixed order. */
int tipk_drug_mix_gather_supported(int p, int q);
int tipk_drug_mix_gather_fwd(const float* xd, int64_t ld_xd, const float* d_norm, const float* h, int64_t ld_h,
                             const int32_t* ptr, const int32_t* src, const float* scale, const int32_t* wg_desc,
                             const int32_t* order /* nullable */, int64_t n_wg,
                             const float* w, int p, int q, int64_t rows, int ne, int cat, float* out, int64_t ld_out,
                             float* mean, tipk_stream_t stream);
int tipk_drug_mix_bwd(const float* g, int64_t ld_g, const float* d_norm, const float* mean, const float* w, int p, int q,
                      int64_t rows, int ne, int cat, float* g_xd, int64_t ld_gxd, float* g_mean, float* g_w,
                      tipk_stream_t stream);

/* Round 6 -- the same forward launch ALSO leaves the first R-GCN layer's row-local products of the rows it finishes
 * (src/layers.py:545 applied to the output of :532-539; reference MyRGCNConv2.forward :159-188, basis-first):
 *     xb[d, b, :d_out] = out[d, :] basis[b]      node-major [.. x n_bases x 32] (rows padded to 32 columns: the operand of
 *                                                tipk_pair_product / tipk_rgcn_pair_grads; columns >= d_out untouched)
 *     xroot[d, :]      = out[d, :] root          [rows x d_out] contiguous
 *   basis [n_bases x cols x d_out], root [cols x d_out] contiguous, cols = cat ? ne + q : ne (a multiple of 4, <= 128),
 *   d_out 16 or 32 (tipk_drug_mix_gather_xb_supported).  v_mfma_f32_16x16x4_f32 on the workgroup's <= 16 rows: a k-ordered
 *   fp32 fma chain per element.  Saves the launch of the two products (9.6 us at BioSNAP for 88 MFLOP). */
int tipk_drug_mix_gather_xb_supported(int p, int q, int ne, int cat, int n_bases, int d_out);
int tipk_drug_mix_gather_xb_fwd(const float* xd, int64_t ld_xd, const float* d_norm, const float* h, int64_t ld_h,
                                const int32_t* ptr, const int32_t* src, const float* scale, const int32_t* wg_desc,
                                const int32_t* order /* nullable */, int64_t n_wg, const float* w, int p, int q, int64_t rows, int ne, int cat, float* out,
                                int64_t ld_out, float* mean, const float* basis, const float* root, int n_bases, int d_out,
                                float* xb, float* xroot, tipk_stream_t stream);

/* Round 6 -- the backward pass of the whole P -> D stage in ONE launch: tipk_drug_mix_bwd + the transposed gather of
 * d mean + the products of GCNConv 2's backward pass (autograd of src/layers.py:526-539 and of PPEncoder.conv2, :394):
 *     g_xd = g[:, :ne] / d_norm                                             as tipk_drug_mix_bwd
 *     g_w_slabs[j] = mean^T g_pd over the j-th share of the rows  [p x q], tipk_pd_stage_bwd_wh_slabs() slabs
 *     g_h[s] = sum_{e in [tptr[s], tptr[s + 1])} tw[e] * (g_pd W^T)[tdst[e]]     per kept source row s (CSR by source row:
 *                                                                                drug ids, 1 / #targets(drug)); never stored
 *     gw[s, :] = (g_h[s] W2) * row_scale[s]        [n_src x c1]; W2 (k < p, n < c1) at w2[k * w2_sk + n * w2_sn]
 *     dw2_slabs[j] = agg[rows of workgroup j]^T g_h    [c1 x p] per row workgroup,  db2_slabs[j] = column sums of g_h  [p]
 *   agg [n_src x c1]: GCNConv 2's aggregated input rows (tipk_gather_sum_lin's first output).  wg_rows int32 [n_row_wg + 1]:
 *   the deal of the source rows to workgroups -- consecutive rows, at most max_rows of them and (unless one row alone has more)
 *   at most max_edges edges per workgroup (tipk_pd_stage_bwd_limits), wg_rows[0] = 0, wg_rows[n_row_wg] = n_src.  The slabs --
 *   n_row_wg of each -- are summed in order by the caller (riders of the next launch).
 *   Supported: tipk_drug_mix_gather_supported(p, q), c1 <= 64, p * c1 <= 4 096. */
int tipk_pd_stage_bwd_supported(int p, int q, int64_t rows, int c1);
int tipk_pd_stage_bwd_limits(int* max_rows, int* max_edges);
int tipk_pd_stage_bwd_wh_slabs(void);
int tipk_pd_stage_bwd(const float* g, int64_t ld_g, const float* d_norm, const float* mean, const float* w, int p, int q,
                      int64_t rows, int ne, int cat, float* g_xd, int64_t ld_gxd, float* g_w_slabs,
                      const int32_t* tptr, const int32_t* tdst, const float* tw, int64_t n_src,
                      const int32_t* wg_rows, int64_t n_row_wg,
                      const float* agg, int64_t ld_agg, int c1, const float* w2, int64_t w2_sk, int64_t w2_sn,
                      const float* row_scale, float* gw, int64_t ld_gw, float* dw2_slabs, float* db2_slabs,
                      tipk_stream_t stream);
/* The same launch with up to 3 ordered slab sums (section 2: tipk_sum_slabs_group) that are READY when it starts riding in it as
 * further workgroups behind the 8 + n_row_wg of the stage, as in tipk_gather_sum_riders: the stage is a chain of L2 round trips
 * on a third of the chip (80 workgroups at BioSNAP), the d att slab sums of both R-GCN layers run next to it instead of behind
 * the dense products of layer 1.  Every sum adds in the order of tipk_sum_slabs_group (bit for bit); a sum with count == 0 is
 * skipped; n_sums == 0 is tipk_pd_stage_bwd itself.  TIPK_EINVAL -- before anything is launched -- for n_sums outside 0 .. 3,
 * sums == NULL with n_sums > 0, or a descriptor tipk_sum_slabs_group refuses. */
int tipk_pd_stage_bwd_riders(const float* g, int64_t ld_g, const float* d_norm, const float* mean, const float* w, int p, int q,
                             int64_t rows, int ne, int cat, float* g_xd, int64_t ld_gxd, float* g_w_slabs,
                             const int32_t* tptr, const int32_t* tdst, const float* tw, int64_t n_src,
                             const int32_t* wg_rows, int64_t n_row_wg,
                             const float* agg, int64_t ld_agg, int c1, const float* w2, int64_t w2_sk, int64_t w2_sn,
                             const float* row_scale, float* gw, int64_t ld_gw, float* dw2_slabs, float* db2_slabs,
                             const struct tipk_slab_sum_desc* sums /* host, [n_sums <= 3], nullable */, int32_t n_sums,
                             tipk_stream_t stream);

/* out[c] = sum_r in[r, c]  (bias gradients of GCNConv).  `scratch` holds >= 256*cols floats.  rows == 0: out = 0, `in` is
 * not read and may be NULL. */
int tipk_col_sum(const float* in, int64_t ld_in, int64_t rows, int64_t cols,
                 float* scratch, float* out, tipk_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * 4. DistMult decoder  score(u,v,r) = sigma( sum_k z[u,k] z[v,k] w[r,k] )
 *    replaces MultiInnerProductDecoder.forward, src/layers.py:590-592 (K9) and its backward.
 *    idx_bytes / et_bytes: 4 (int32) or 8 (int64, the reference's dtype) -- read in place.
 *    tipk_distmult_loss and tipk_typed_negative_sampling also take idx_bytes = 2: PACKED pairs, one uint32 word
 *    u | v << 16 per triple in the `_u` array (the `_v` pointer is unused; n_nodes <= 65535) -- the static positives
 *    are narrowed once, the sampler emits its negatives in this form: 66 MB of ids per BioSNAP step instead of 266 MB.
 */
int tipk_distmult_fwd(const float* z, int64_t n_nodes, int k, const float* rel_w, int64_t n_rel,
                      const void* idx_u, const void* idx_v, int idx_bytes,
                      const void* edge_type, int et_bytes, int64_t n_triples,
                      int sigmoid, float* score, tipk_stream_t stream);

/* g_z [n_nodes x k] and g_w [n_rel x k] are ACCUMULATED into (caller zeroes them);
 * `score` is the forward output when sigmoid != 0 (unused otherwise).
 * tasks (nullable): int32 [n_tasks, 4] = (relation, begin, end, pos_weight) -- ranges of AT MOST 2048
 * positions that share one relation, covering [0, n_triples), largest first.  pos_weight is read by
 * tipk_distmult_loss only: the weight (1, or 2 / 0) of the task's POSITIVE triples -- when every relation
 * lists each pair in both directions ([u<v half | mirrored half], src/utils.py:35-65) the host may give
 * the first half weight 2 and the mirrored half weight 0 (identical scores and gradients): the objective
 * and all gradients are unchanged, a quarter of the work disappears.  TIP's triples are grouped by relation
 * (src/utils.py:57-63), so the host builds this once; with it, z and rel_w on 16-byte addresses, k a power of two in 4..64,
 * n_nodes <= 65 535 and the kernel's LDS images inside 158 KB -- per node (k + 1) 64-bit words of the fixed-point d z image
 * and (k + 4) floats of the z image (each image rounded up to 16 bytes), plus 16 k + 16 floats of reduction space and 16 KB
 * of staged ids: n_nodes <= 2 015 for k = 4, 668 for k = 16, 178 for k = 64 -- the LDS-resident task kernel runs,
 * otherwise the generic one (tipk_distmult_route names the route; ask it, do not copy this).
 *
 * Non-finite rule of tipk_distmult_bwd.  No element of g_z / g_w that the exact gradient makes NaN or infinite comes out
 * finite.  The generic routes add float terms: what is finite in exact arithmetic (and in fp32 range) stays a rounded
 * number.  The task route scales its fixed-point d z image by a bound, 4 max|z| max|w| sum |g_score| over the positions of
 * ONE workgroup; where that bound is not a finite float -- a NaN or an infinity anywhere in z or rel_w, or in a g_score of
 * that workgroup's tasks, or finite g_score whose magnitudes sum past FLT_MAX -- the workgroup adds NaN to EVERY element of
 * g_z: it poisons more than the exact gradient does, never less (the fused objective does the same for z and rel_w).
 * g_w is a float sum on every route. */
int tipk_distmult_bwd(const float* g_score, const float* score,
                      const float* z, int64_t n_nodes, int k, const float* rel_w, int64_t n_rel,
                      const void* idx_u, const void* idx_v, int idx_bytes,
                      const void* edge_type, int et_bytes, int64_t n_triples,
                      int sigmoid, const int32_t* tasks, int64_t n_tasks,
                      float* g_z, float* g_w, tipk_stream_t stream);

/* The route of tipk_distmult_bwd / tipk_distmult_loss for a shape: a pure host query, and the ONE decision the two entries
 * take themselves (options apply: "dm_task_kernel").
 *   mode          TIPK_DM_MODE_BWD, _LOSS (g_z / g_w given) or _LOSS_NOGRAD (objective only)
 *   has_tasks     a task table is passed (non-NULL, 0 < n_tasks < 2^31);  has_workspace: tipk_distmult_loss's workspace
 *   idx_bytes     4, 8, or 2 (packed pairs, the loss only);  aligned16: z and rel_w both on 16-byte addresses
 * -> TIPK_DM_ROUTE_GENERIC_GLOBAL  one thread per triple, d z by global float atomics (n_nodes k 4 B > 96 KB, or no gradients)
 *    TIPK_DM_ROUTE_GENERIC_LDS     the same kernel, d z in a per-workgroup float LDS image (n_nodes k 4 B <= 96 KB)
 *    TIPK_DM_ROUTE_TASK            distmult_task_kernel: tasks, z and the fixed-point d z image in LDS
 *    TIPK_DM_ROUTE_OBJECTIVE       distmult_objective_kernel (the loss with tasks, a workspace and k in {4, 8, 16})
 *    TIPK_EUNSUPPORTED             packed pairs outside the objective kernel;  TIPK_EINVAL: no such mode / id width / shape.
 * (tipk_distmult_loss_store additionally needs a workspace route: TIPK_EUNSUPPORTED on the generic ones.) */
#define TIPK_DM_MODE_BWD 0
#define TIPK_DM_MODE_LOSS 1
#define TIPK_DM_MODE_LOSS_NOGRAD 2
#define TIPK_DM_ROUTE_GENERIC_GLOBAL 0
#define TIPK_DM_ROUTE_GENERIC_LDS 1
#define TIPK_DM_ROUTE_TASK 2
#define TIPK_DM_ROUTE_OBJECTIVE 3
int tipk_distmult_route(int64_t n_nodes, int k, int mode, int has_tasks, int has_workspace, int idx_bytes, int aligned16);

/* Fused training objective of TIP.forward (src/layers.py:335-340, K9+K10): one pass over the
 * positive triples and their negatives (same relation per position):
 *   loss = -mean log(sigma(pos)+1e-13) - mean log(1-sigma(neg)+1e-13)
 * loss_out[0] += loss (caller zeroes); if g_z/g_w are non-NULL they receive d loss / d z, d w
 * (accumulated; caller zeroes), so the backward pass is a scale by the upstream scalar.
 *
 * workspace (nullable; tipk_distmult_workspace_bytes(...) bytes, 8-byte aligned, ZEROED before its first use;
 * the call leaves it zeroed): with it -- and a task table, i.e. on the LDS-resident fast kernel -- the sums across
 * workgroups of loss, d z and d w are 64-bit fixed-point integer atomics (exact, order-independent) converted by
 * a finalize launch: the objective and its gradients are BITWISE REPRODUCIBLE from run to run (the float
 * atomics of the default path differ at the 1e-7 level with the arrival order of 256 workgroups).
 * With k in {4, 8, 16} this path runs distmult_objective_kernel: one lane evaluates a position (ids straight from global
 * memory, sigma / log / quotient on the hardware transcendental units), the gradient terms are scattered with k lanes per
 * row of the LDS image, and every term is converted to fixed point with a PER-TERM scale (|term| <= 4 zmax wmax / n:
 * one multiply, one round, one 32-bit convert instead of a double-precision sequence); option "dm_task_kernel" = 1
 * keeps the k/4-lanes-per-position kernel of round 2 for A/B runs. */
int64_t tipk_distmult_workspace_bytes(int64_t n_nodes, int k, int64_t n_rel);
int tipk_distmult_loss(const float* z, int64_t n_nodes, int k, const float* rel_w, int64_t n_rel,
                       const void* pos_u, const void* pos_v, const void* neg_u, const void* neg_v,
                       int idx_bytes, const void* edge_type, int et_bytes, int64_t n_triples,
                       const int32_t* tasks, int64_t n_tasks,
                       float* loss_out, float* g_z, float* g_w, void* workspace, tipk_stream_t stream);
/* Same, but loss_out / g_z / g_w are OVERWRITTEN (they need not be zeroed: three fill launches less per training
 * step; the bits are those of tipk_distmult_loss on zeroed outputs).  Only the workspace path can do that (its finalize
 * launch visits every output element): TIPK_EUNSUPPORTED otherwise, nothing launched. */
int tipk_distmult_loss_store(const float* z, int64_t n_nodes, int k, const float* rel_w, int64_t n_rel,
                             const void* pos_u, const void* pos_v, const void* neg_u, const void* neg_v,
                             int idx_bytes, const void* edge_type, int et_bytes, int64_t n_triples,
                             const int32_t* tasks, int64_t n_tasks,
                             float* loss_out, float* g_z, float* g_w, void* workspace, tipk_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * 4b. NNDecoder triple scoring (reference src/layers.py:598-637, the paper's DR-NN ablation; SURVEY
 *     section 8(f) item 1):  score[e] = sigma( s1[u_e, r_e] + s2[v_e, r_e] )  with the dense tables
 *     s1 = relu(z w1_l1) w1_l2^T and s2 = relu(z w2_l1) w2_l2^T ([n_nodes x n_rel], row stride ld)
 *     produced by tipk_gemm_f32.  bwd ACCUMULATES d s1 / d s2 (caller zeroes) with float atomics.
 */
int tipk_pair_table_fwd(const float* s1, const float* s2, int64_t ld,
                        const void* idx_u, const void* idx_v, int idx_bytes,
                        const void* edge_type, int et_bytes, int64_t n_triples,
                        int sigmoid, float* score, tipk_stream_t stream);
int tipk_pair_table_bwd(const float* g_score, const float* score, int64_t ld,
                        const void* idx_u, const void* idx_v, int idx_bytes,
                        const void* edge_type, int et_bytes, int64_t n_triples,
                        int sigmoid, float* g_s1, float* g_s2, tipk_stream_t stream);
/*     The fused TIP objective on the tables (src/layers.py:335-340 with this decoder, model/ddm-nn.py:65-102):
 *        loss = -mean log(sigma(x_pos) + eps) - mean log(1 - sigma(x_neg) + eps),  x = S1[u, r] + S2[v, r]
 *     on TRANSPOSED tables s1t / s2t [n_rel][ld] (row r = every node's score under relation r: w_l2 . relu(z w_l1)^T from
 *     tipk_gemm_f32).  pos_pairs / neg_pairs [n_positions]: u | v << 16 per triple (n_nodes <= 65 535), both grouped by
 *     relation with the SAME blocks rel_ptr [n_rel + 1] (the sampler's layout); order [n_rel]: the relations by decreasing
 *     block size (launch order of the per-relation workgroups).  Outputs: loss_parts [n_rel][2] (double) = a relation's
 *     sums of log(sigma_pos + eps) and log(1 - sigma_neg + eps): loss = -(sum of all) / n_positions; g_s1t / g_s2t
 *     [n_rel][ld] (both or neither; columns < n_nodes of EVERY row are written) = d loss / d S1^T, d S2^T, accumulated in
 *     LDS as 64-bit fixed point: no atomics on global memory, bitwise reproducible. */
int tipk_pair_table_loss(const float* s1t, const float* s2t, int64_t ld, int64_t n_nodes, int64_t n_rel,
                         const uint32_t* pos_pairs, const uint32_t* neg_pairs, const int64_t* rel_ptr,
                         const int32_t* order, int64_t n_positions, float eps, double* loss_parts,
                         float* g_s1t /* nullable */, float* g_s2t /* nullable */, tipk_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * 4c. DistMult screen: the k best UNSEEN candidates of a query, ranked on the logit
 *        s(u, v, r) = sum_k z[u,k] z[v,k] w[r,k]
 *     (serving; no reference call site: the reference ranks side effects per relation, never the pairs themselves).
 *
 *   z [n_nodes x dim], rel_w [n_rel x dim] fp32 row-major (z 16-byte aligned).  queries: HOST int32 [n_q][2] =
 *   (relation r, drug u); u = -1 is a RELATION query: every unordered pair u < v (no self pairs; DistMult is symmetric,
 *   so (u, v) and (v, u) are one candidate); u >= 0 is a DRUG query: every partner v != u, returned as (u, v).
 *   known_keys / known_ptr (nullable together; device): int64 keys u*n+v sorted inside each relation, relation r's block
 *   [known_ptr[r], known_ptr[r+1]) -- the sampler's pos_key_sorted / rel_ptr layout.  A candidate is dropped when u*n+v
 *   OR v*n+u is a key of its relation (lists that hold one direction only are handled).
 *   Output per query (device): out_score fp32 [n_q x k] = LOGITS (sigma saturates to 1.0 in fp32 above ~17, which would
 *   turn the top of a list into ties), out_u / out_v int32 [n_q x k]; order: descending logit, ties by ascending key
 *   u*n+v; a query with fewer than k candidates is padded with (-inf, -1, -1).
 *   Numerics: each logit is fp32, a = z[u,k] * w[r,k] rounded, then fmaf(a, z[v,k], acc) for k ascending from 0 -- one
 *   value per pair on every route and split; the result is BITWISE repeatable (the merge across workgroups is by rank).
 *   A candidate whose logit is NaN is never returned; +inf and -inf logits rank as values, so a -inf candidate is an entry
 *   (valid u and v, score -inf) ahead of the padding, not padding.
 *   Filter routes: an LDS bitmap of the relation's known pairs when n_nodes^2 bits fit in 64 KB
 *   (tipk_distmult_screen_bitmap_route), binary search in the keys otherwise or under option "screen_search"; same bits.
 *   Supported (tipk_distmult_screen_supported): 1 <= n_nodes <= 46 340 (n^2 < 2^31), dim % 4 == 0 in 4..256, 1 <= k <= 1 024.
 *   Status: TIPK_EINVAL -- before anything is launched or written -- for k <= 0, a relation outside [0, n_rel), a drug
 *   outside [-1, n_nodes), keys without offsets (or the reverse), a NULL pointer; then TIPK_EUNSUPPORTED outside the
 *   supported range; TIPK_OK implies correct numbers.
 *   workspace: tipk_distmult_screen_workspace_bytes(n_nodes, dim, n_q, k) bytes, 16-byte aligned (-1: unsupported).
 *   This entry SYNCHRONISES `stream` once: it copies the host query list into the workspace and waits for the copy, so
 *   the caller may reuse `queries` on return (not for stream capture).
 */
int     tipk_distmult_screen_supported(int64_t n_nodes, int dim, int k);
int64_t tipk_distmult_screen_workspace_bytes(int64_t n_nodes, int dim, int64_t n_q, int k);
int     tipk_distmult_screen_bitmap_route(int64_t n_nodes);     /* 1 = the LDS bitmap filters this node count (options apply) */
int     tipk_distmult_screen(const float* z, int64_t n_nodes, int dim, const float* rel_w, int64_t n_rel,
                             const int32_t* queries /* host */, int64_t n_q,
                             const int64_t* known_keys /* nullable */, const int64_t* known_ptr /* [n_rel+1], nullable */,
                             int k, float* out_score, int32_t* out_u, int32_t* out_v, void* workspace, tipk_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * 4d. Pair top-k: the k best relations (side effects) of every pair of a list, known ones dropped, ranked on the logit
 *     (serving; the transposed question of 4c; no reference call site: `TIP.pred` scores given triples only).
 *
 *   pair_u / pair_v: DEVICE int32 [n_pairs].  The candidates of pair (u, v) are all relations r in [0, n_rel); self pairs
 *   and repeated pairs are legal and are scored like any other.  A pair with an index outside [0, n_nodes) gets a fully
 *   padded row and reads nothing out of bounds (device data cannot be validated on the host without a sync).
 *   DistMult (tipk_distmult_pair_topk): z [n_nodes x dim], rel_w [n_rel x dim] fp32 row-major (rel_w 16-byte aligned).
 *   Each logit is fp32: h_k = z[u,k] * z[v,k] rounded, then acc = fmaf(h_k, w[r,k], acc) for k ascending from 0 -- one
 *   value per pair on every route, and (u, v) and (v, u) give identical bits.
 *   Table variant (tipk_pair_table_pair_topk; the NN decoder of 4b): node-major tables s1, s2 [n_nodes x ld], ld >= n_rel,
 *   as NNDecoder.forward forms them; the logit is the single fp32 add s1[u,r] + s2[v,r]; NOT symmetric in (u, v).
 *   Known filter, pair-major (nullable together; device): known_pair_keys int64 [n_known_pairs], strictly ascending keys
 *   min(u,v)*n_nodes + max(u,v); known_pair_ptr int64 [n_known_pairs + 1]; known_rel int32, ascending relation ids inside
 *   each pair's block [known_pair_ptr[i], known_pair_ptr[i+1]).  A relation listed for the pair's UNORDERED key is dropped
 *   in either pair direction, for both decoders.  One search per pair finds the block; the block is then merged into a
 *   bitmap of the wavefront: never a search per (pair, relation).
 *   Output per pair (device): out_score fp32 [n_pairs x k] = LOGITS (for the reason 4c gives: sigma saturates in fp32),
 *   out_rel int32 [n_pairs x k]; order: descending logit, ties by ascending relation id; a row with fewer than k candidates
 *   is padded with (-inf, -1).  A NaN logit is never returned.  The result is a set fixed by that total order and is
 *   BITWISE repeatable.
 *   Routes (DistMult): rel_w is staged in LDS once per workgroup when it fits beside the wavefronts' lists
 *   (tipk_distmult_pair_topk_lds_route: 1 097 x 16 does), and streamed through LDS in tiles, one pass per block of 16
 *   pairs, otherwise or under option "pair_topk_stream"; same bits.
 *   Supported: 1 <= n_nodes <= 46 340, dim % 4 == 0 in 4..256 (DistMult), 1 <= n_rel <= 65 536, 1 <= k <= 128.
 *   Status: TIPK_EINVAL -- before anything is launched or written -- for k <= 0, a negative size, n_nodes or n_rel < 1,
 *   ld < n_rel, a NULL required pointer (with n_pairs > 0), known arrays given only in part; then TIPK_EUNSUPPORTED outside
 *   the supported range; n_pairs == 0 is TIPK_OK with no launch; TIPK_OK implies correct numbers.
 *   workspace: tipk_distmult_pair_topk_workspace_bytes(...) bytes (-1: unsupported).  Every list lives in LDS, so this is
 *   0 for every supported shape today and `workspace` may then be NULL.
 *   Unlike 4c nothing lives in host memory: these entries do NOT synchronise and may be captured into a hipGraph.
 */
int     tipk_distmult_pair_topk_supported(int64_t n_nodes, int dim, int64_t n_rel, int k);
int64_t tipk_distmult_pair_topk_workspace_bytes(int64_t n_nodes, int dim, int64_t n_rel, int64_t n_pairs, int k);
int     tipk_distmult_pair_topk_lds_route(int dim, int64_t n_rel);   /* 1 = rel_w is staged in LDS once (options apply) */
int     tipk_distmult_pair_topk(const float* z, int64_t n_nodes, int dim, const float* rel_w, int64_t n_rel,
                                const int32_t* pair_u, const int32_t* pair_v /* device */, int64_t n_pairs,
                                const int64_t* known_pair_keys, const int64_t* known_pair_ptr, const int32_t* known_rel,
                                int64_t n_known_pairs /* nullable together */,
                                int k, float* out_score, int32_t* out_rel, void* workspace, tipk_stream_t stream);
int     tipk_pair_table_pair_topk_supported(int64_t n_nodes, int64_t n_rel, int k);
int     tipk_pair_table_pair_topk(const float* s1, const float* s2, int64_t ld, int64_t n_nodes, int64_t n_rel,
                                  const int32_t* pair_u, const int32_t* pair_v /* device */, int64_t n_pairs,
                                  const int64_t* known_pair_keys, const int64_t* known_pair_ptr, const int32_t* known_rel,
                                  int64_t n_known_pairs /* nullable together */,
                                  int k, float* out_score, int32_t* out_rel, tipk_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * 4e. Regimen top-k: the k best relations (side effects) of every drug LIST, aggregated over the list's pairs, with the pair
 *     that drives each (serving; polypharmacy beyond one pair; no reference call site).
 *
 *   Regimen lists, CSR, DEVICE: reg_drugs int32 [n_entries], reg_ptr int64 [n_regimens + 1].  Regimen g is the list
 *   d_0 .. d_{m-1} = reg_drugs[reg_ptr[g] .. reg_ptr[g+1]); its pairs are the POSITION pairs (i, j), i < j, in lexicographic
 *   order, with u = d_i and v = d_j.  Equal ids at two positions are scored as a self pair, as 4d does.
 *   Logit of a triple (pair, r): exactly that of 4d.  DistMult: h_k = z[u,k] * z[v,k] rounded once, then
 *   acc = fmaf(h_k, w[r,k], acc) for k ascending from 0.  Table variant: the single fp32 add s1[u,r] + s2[v,r], u being the
 *   EARLIER list position.
 *   Skipped triples: a triple contributes nothing when it is KNOWN -- listed for the pair's unordered key in the pair-major
 *   lists (known_pair_keys, known_pair_ptr, known_rel) of 4d, nullable together -- or when its logit is NaN.  A relation
 *   whose every triple is skipped is not a candidate.
 *   Aggregate per (regimen, relation), chosen by `aggregate`:
 *     TIPK_REGIMEN_MAX       A = the largest contributing logit; exact: the score is bit-identical to that triple's 4d logit.
 *     TIPK_REGIMEN_NOISY_OR  A = sum over the contributing triples, in pair order, in fp32 (A starts at 0.0f and each term is
 *                            added with one rounding), of
 *                                softplus(s) = fmaxf(s, 0) + log1pf(expf(-fabsf(s)))
 *                            which is -log(1 - P) of the noisy-or probability P = 1 - prod (1 - sigma(s)).  The ranking is
 *                            on A, not on P: P saturates to 1 in fp32.  P = -expm1(-A).
 *   Driver pair, for either aggregate: the positions (i, j) of the contributing triple with the largest logit, ties to the
 *   first in pair order, packed i | j << 16 into an int32.
 *   Output per regimen (device): the k best relations by (A descending, relation id ascending) in out_score fp32
 *   [n_regimens x k], out_rel int32 [n_regimens x k], out_pair int32 [n_regimens x k]; a row with fewer than k candidates
 *   is padded with (-inf, -1, -1).  A regimen with fewer than 2 entries, with more than tipk_regimen_max_drugs() entries
 *   (64) or with any drug id outside [0, n_nodes) gets a fully padded row and nothing of it is read out of bounds.
 *   The result is a set fixed by that total order and is BITWISE repeatable (the noisy-or sum has a fixed order).
 *   Routes (DistMult): rel_w is staged in LDS once per workgroup when it fits beside the wavefronts' state
 *   (tipk_distmult_regimen_topk_lds_route: 1 097 x 16 does); otherwise, or under option "regimen_global", every lane reads
 *   its rows from global memory; same bits.
 *   Supported: as 4d -- 1 <= n_nodes <= 46 340, dim % 4 == 0 in 4..256 (DistMult; rel_w 16-byte aligned), 1 <= n_rel <=
 *   65 536, 1 <= k <= 128; regimen length 2..tipk_regimen_max_drugs().
 *   Status: TIPK_EINVAL -- before anything is launched or written -- for k <= 0, a negative size, n_nodes or n_rel < 1,
 *   ld < n_rel, an unknown `aggregate`, a NULL required pointer (reg_ptr, reg_drugs, the tables, the three outputs; with
 *   n_regimens > 0), known arrays given only in part; then TIPK_EUNSUPPORTED outside the supported range; n_regimens == 0
 *   is TIPK_OK with no launch; TIPK_OK implies correct numbers.
 *   workspace: tipk_distmult_regimen_topk_workspace_bytes(...) bytes (-1: unsupported); every list lives in LDS, so this is
 *   0 for every supported shape today and `workspace` may then be NULL.
 *   Nothing lives in host memory: these entries do NOT synchronise and may be captured into a hipGraph.
 */
#define TIPK_REGIMEN_MAX      0
#define TIPK_REGIMEN_NOISY_OR 1
int     tipk_regimen_max_drugs(void);
int     tipk_distmult_regimen_topk_supported(int64_t n_nodes, int dim, int64_t n_rel, int k);
int64_t tipk_distmult_regimen_topk_workspace_bytes(int64_t n_nodes, int dim, int64_t n_rel, int64_t n_regimens, int k);
int     tipk_distmult_regimen_topk_lds_route(int dim, int64_t n_rel);   /* 1 = rel_w is staged in LDS once (options apply) */
int     tipk_distmult_regimen_topk(const float* z, int64_t n_nodes, int dim, const float* rel_w, int64_t n_rel,
                                   const int32_t* reg_drugs, const int64_t* reg_ptr /* device */, int64_t n_regimens,
                                   const int64_t* known_pair_keys, const int64_t* known_pair_ptr, const int32_t* known_rel,
                                   int64_t n_known_pairs /* nullable together */,
                                   int aggregate, int k, float* out_score, int32_t* out_rel, int32_t* out_pair,
                                   void* workspace, tipk_stream_t stream);
int     tipk_pair_table_regimen_topk_supported(int64_t n_nodes, int64_t n_rel, int k);
int     tipk_pair_table_regimen_topk(const float* s1, const float* s2, int64_t ld, int64_t n_nodes, int64_t n_rel,
                                     const int32_t* reg_drugs, const int64_t* reg_ptr /* device */, int64_t n_regimens,
                                     const int64_t* known_pair_keys, const int64_t* known_pair_ptr, const int32_t* known_rel,
                                     int64_t n_known_pairs /* nullable together */,
                                     int aggregate, int k, float* out_score, int32_t* out_rel, int32_t* out_pair,
                                     tipk_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * 4f. Pair rank: the filtered rank of given relations (held-out side effects) among all relations of their pair, on the
 *     logit (evaluation of what 4d serves: filtered MRR / Hits@k; no reference call site).
 *
 *   Input, pair-major, DEVICE: pair_u / pair_v int32 [n_pairs]; tgt_ptr int64 [n_pairs + 1], tgt_rel int32 [n_tgt]: pair p
 *   owns the targets tgt_rel[tgt_ptr[p] : tgt_ptr[p+1]].  Targets may come in any order, may repeat, and a pair may have
 *   none.  n_tgt is the length of tgt_rel (= tgt_ptr[n_pairs]); positions outside [0, n_tgt) are neither read nor written.
 *   Logits: bit for bit those of 4d.  DistMult: h_k = z[u,k] * z[v,k] rounded, then acc = fmaf(h_k, w[r,k], acc) for k
 *   ascending from 0; (u, v) and (v, u) give identical bits.  Table variant: the single fp32 add s1[u,r] + s2[v,r]; NOT
 *   symmetric in (u, v).
 *   Candidates of a target t of pair (u, v): every relation in [0, n_rel) except those listed for the pair's UNORDERED key
 *   in the pair-major known lists of 4d (nullable together).  The target itself is never dropped, listed or not.
 *   Rank (1-based): rank = 1 + #{candidates c != t : logit[c] > logit[t] or (logit[c] == logit[t] and c < t)} -- the total
 *   order of 4d, so rank - 1 is the position the pair top-k gives the same relation under the same filter (with t taken
 *   off the known list).  A candidate whose logit is NaN beats nothing.
 *   Output per target (device): out_rank int32 [n_tgt]; out_logit fp32 [n_tgt] (nullable) = the target's logit.
 *   Not ranked -- rank 0, logit NaN, nothing read out of bounds: a target whose logit is NaN, a target outside [0, n_rel),
 *   a pair with an index outside [0, n_nodes).
 *   Routes (DistMult): rel_w is staged in LDS once per workgroup when it fits (tipk_distmult_pair_rank_lds_route: 1 097 x 16
 *   does); otherwise, or under option "pair_rank_stream", every lane reads its rows from global memory; same bits.
 *   Supported: as 4d without k -- 1 <= n_nodes <= 46 340, dim % 4 == 0 in 4..256 (DistMult; rel_w 16-byte aligned),
 *   1 <= n_rel <= 65 536; any number of targets per pair.
 *   Status: TIPK_EINVAL -- before anything is launched or written -- for a negative size, n_nodes or n_rel < 1, ld < n_rel,
 *   a NULL required pointer (the lists, the tables, out_rank; with n_pairs > 0 and n_tgt > 0), known arrays given only in
 *   part; then TIPK_EUNSUPPORTED outside the supported range; n_pairs == 0 or n_tgt == 0 is TIPK_OK with no launch; TIPK_OK
 *   implies correct numbers.
 *   No workspace.  Nothing lives in host memory: these entries do NOT synchronise, may be captured into a hipGraph and are
 *   BITWISE repeatable (integer counts; no atomics on global memory).
 */
int     tipk_distmult_pair_rank_supported(int64_t n_nodes, int dim, int64_t n_rel);
int     tipk_distmult_pair_rank_lds_route(int dim, int64_t n_rel);   /* 1 = rel_w is staged in LDS once (options apply) */
int     tipk_distmult_pair_rank(const float* z, int64_t n_nodes, int dim, const float* rel_w, int64_t n_rel,
                                const int32_t* pair_u, const int32_t* pair_v /* device */, int64_t n_pairs,
                                const int64_t* tgt_ptr, const int32_t* tgt_rel /* device */, int64_t n_tgt,
                                const int64_t* known_pair_keys, const int64_t* known_pair_ptr, const int32_t* known_rel,
                                int64_t n_known_pairs /* nullable together */,
                                int32_t* out_rank, float* out_logit /* nullable */, tipk_stream_t stream);
int     tipk_pair_table_pair_rank_supported(int64_t n_nodes, int64_t n_rel);
int     tipk_pair_table_pair_rank(const float* s1, const float* s2, int64_t ld, int64_t n_nodes, int64_t n_rel,
                                  const int32_t* pair_u, const int32_t* pair_v /* device */, int64_t n_pairs,
                                  const int64_t* tgt_ptr, const int32_t* tgt_rel /* device */, int64_t n_tgt,
                                  const int64_t* known_pair_keys, const int64_t* known_pair_ptr, const int32_t* known_rel,
                                  int64_t n_known_pairs /* nullable together */,
                                  int32_t* out_rank, float* out_logit /* nullable */, tipk_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * 4g. Partner rank: the filtered rank of given partners (held-out drugs) among all drugs, per (relation, drug) query, on the
 *     logit (evaluation of what the drug queries of 4c serve: entity-ranking filtered MRR / Hits@k; no reference call site).
 *
 *   Input, query-major, DEVICE: q_rel / q_drug int32 [n_q]; tgt_ptr int64 [n_q + 1], tgt_node int32 [n_tgt]: query
 *   q = (r, u) owns the target partners tgt_node[tgt_ptr[q] : tgt_ptr[q+1]].  Targets may come in any order, may repeat, and
 *   a query may have none.  n_tgt is the length of tgt_node (= tgt_ptr[n_q]); tgt_ptr is clamped to it: positions outside
 *   [0, n_tgt) are neither read nor written.
 *   Logits: bit for bit those of a 4c drug query.  DistMult: a_k = z[u,k] * w[r,k] rounded once, then
 *   acc = fmaf(a_k, z[c,k], acc) for k ascending from 0.  This is NOT symmetric in (u, c): the queried drug is the one
 *   multiplied with w first, and (r, u) ranking c may differ in the last bit from (r, c) ranking u.  Table variant
 *   (tipk_pair_table_partner_rank; the NN decoder of 4b): the RELATION-major tables s1t, s2t [n_rel x ld], ld >= n_nodes,
 *   as NNDecoder.objective forms them for tipk_pair_table_loss; the logit is the single fp32 add s1t[r,u] + s2t[r,c]; a
 *   query's candidates are one coalesced row.
 *   Candidates of a target t of query (r, u): every drug c in [0, n_nodes) with c != u, except those with u*n+c OR c*n+u a
 *   key of relation r in the relation-major lists of 4c (known_keys sorted inside each relation, known_ptr [n_rel + 1];
 *   nullable together; lists that hold one direction only are handled).  The target itself is never dropped, listed or not.
 *   Rank (1-based): rank = 1 + #{candidates c != t : logit[c] > logit[t] or (logit[c] == logit[t] and c < t)} -- the total
 *   order of 4c for a fixed u (key u*n+v ascending), so rank - 1 is the position a 4c drug query (r, u) gives (u, t) under
 *   the same filter (with t taken off the known list).  A candidate whose logit is NaN beats nothing.
 *   Output per target (device): out_rank int32 [n_tgt]; out_logit fp32 [n_tgt] (nullable) = the target's logit.
 *   Not ranked -- rank 0, logit NaN, nothing read out of bounds: r outside [0, n_rel), u or t outside [0, n_nodes), t == u
 *   (the screen has no self pairs), a target whose logit is NaN.
 *   Routes (DistMult): z is staged in LDS once per workgroup when it fits beside the wavefronts' state
 *   (tipk_distmult_partner_rank_lds_route: 645 x 16 does); otherwise, or under option "partner_rank_global", every lane reads
 *   its rows from global memory; same bits.
 *   Filter scheme: the keys [u*n, (u+1)*n) of relation r (two searches) are merged into a bitmap of the wavefront; the
 *   reverse keys c*n+u are searched per candidate, only for a candidate that beats the weakest target at hand.
 *   Supported: as 4c/4d -- 1 <= n_nodes <= 46 340, dim % 4 == 0 in 4..256 (DistMult; z 16-byte aligned),
 *   1 <= n_rel <= 65 536; any number of targets per query.
 *   Status: TIPK_EINVAL -- before anything is launched or written -- for a negative size, n_nodes or n_rel < 1,
 *   ld < n_nodes, a NULL required pointer (the lists, the tables, out_rank; with n_q > 0 and n_tgt > 0), keys without
 *   offsets or the reverse; then TIPK_EUNSUPPORTED outside the supported range; n_q == 0 or n_tgt == 0 is TIPK_OK with no
 *   launch; TIPK_OK implies correct numbers.
 *   No workspace.  Nothing lives in host memory: these entries do NOT synchronise, may be captured into a hipGraph and are
 *   BITWISE repeatable (integer counts; no atomics on global memory).
 */
int     tipk_distmult_partner_rank_supported(int64_t n_nodes, int dim, int64_t n_rel);
int     tipk_distmult_partner_rank_lds_route(int64_t n_nodes, int dim);   /* 1 = z is staged in LDS once (options apply) */
int     tipk_distmult_partner_rank(const float* z, int64_t n_nodes, int dim, const float* rel_w, int64_t n_rel,
                                   const int32_t* q_rel, const int32_t* q_drug /* device */, int64_t n_q,
                                   const int64_t* tgt_ptr, const int32_t* tgt_node /* device */, int64_t n_tgt,
                                   const int64_t* known_keys /* nullable */, const int64_t* known_ptr /* [n_rel+1], nullable */,
                                   int32_t* out_rank, float* out_logit /* nullable */, tipk_stream_t stream);
int     tipk_pair_table_partner_rank_supported(int64_t n_nodes, int64_t n_rel);
int     tipk_pair_table_partner_rank(const float* s1t, const float* s2t, int64_t ld, int64_t n_nodes, int64_t n_rel,
                                     const int32_t* q_rel, const int32_t* q_drug /* device */, int64_t n_q,
                                     const int64_t* tgt_ptr, const int32_t* tgt_node /* device */, int64_t n_tgt,
                                     const int64_t* known_keys /* nullable */, const int64_t* known_ptr /* [n_rel+1], nullable */,
                                     int32_t* out_rank, float* out_logit /* nullable */, tipk_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * 4h. Screen rank: the filtered rank of given drug pairs (held-out pairs) among ALL unordered pairs, per relation query, on
 *     the logit (evaluation of what the relation queries of 4c serve: "Hits@50 of relation r" is how many held-out pairs the
 *     screen's 50 best show -- Decagon's AP@50 idea; no reference call site).  DistMult only, as 4c.
 *
 *   Input, query-major, DEVICE: q_rel int32 [n_q]; tgt_ptr int64 [n_q + 1], tgt_u / tgt_v int32 [n_tgt]: query q is relation
 *   q_rel[q] and owns the target pairs tgt_u/tgt_v[tgt_ptr[q] : tgt_ptr[q+1]].  Targets may come in any order, may repeat, a
 *   query may have none, and two queries may name the same relation.  tgt_ptr is clamped to n_tgt: positions outside
 *   [0, n_tgt) are neither read nor written.
 *   Pair form: a target (u, v) is ranked as the unordered pair (a, b) = (min, max) with key a*n+b; (u, v) and (v, u) give the
 *   same rank and the same logit bits.
 *   Logits: bit for bit those of a 4c relation query -- x_k = z[a,k] * w[r,k] rounded once, then acc = fmaf(x_k, z[b,k], acc)
 *   for k ascending from 0 -- for the candidates and, by the same arithmetic, for the targets.
 *   Candidates of relation r: every pair a < b < n_nodes with neither a*n+b nor b*n+a a key of r in the relation-major lists
 *   of 4c (known_keys sorted inside each relation, known_ptr [n_rel + 1]; nullable together; lists that hold one direction
 *   only are handled; keys outside [0, n^2) are ignored).  Whether a target is itself listed changes only whether it is a
 *   candidate for OTHER targets; it is never counted against itself.
 *   Rank (1-based): rank(t) = 1 + #{candidates c != t : L[c] > L[t] or (L[c] == L[t] and key(c) < key(t))} -- the total order
 *   of 4c.  A candidate whose logit is NaN beats nothing.
 *   Relation to 4c: run the 4c relation query (r, -1) under the same known list.  A target that is not listed sits at
 *   position rank - 1 of that list (with the same logit bits); for a listed target, rank - 1 is the number of list entries
 *   that are better than it.
 *   Output per target (device): out_rank int32 [n_tgt]; out_logit fp32 [n_tgt] (nullable) = the target's logit.
 *   Not ranked -- rank 0, logit NaN, nothing read out of bounds: q_rel[q] outside [0, n_rel) (every target of that query),
 *   u or v outside [0, n_nodes), u == v, a target whose logit is NaN.
 *   Filter routes: the LDS bitmap of the relation's known pairs exactly where tipk_distmult_screen_bitmap_route(n_nodes) says
 *   so, binary search in the keys otherwise or under option "screen_search"; same bits.
 *   Passes: a workgroup ranks tipk_distmult_screen_rank_chunk() targets of its query per pass over its candidates; a query
 *   with more targets takes several passes (any number of targets per query).
 *   Supported (tipk_distmult_screen_rank_supported): 1 <= n_nodes <= 46 340, dim % 4 == 0 in 4..256 (z 16-byte aligned),
 *   1 <= n_rel <= 65 536.
 *   Status: TIPK_EINVAL -- before anything is launched or written -- for a negative size, n_nodes, n_rel or dim < 1, a NULL
 *   required pointer (z, rel_w, the lists, out_rank; with n_q > 0 and n_tgt > 0), keys without offsets or the reverse, a NULL
 *   workspace where tipk_distmult_screen_rank_workspace_bytes > 0; then TIPK_EUNSUPPORTED outside the supported range or for
 *   a misaligned z; n_q == 0 or n_tgt == 0 is TIPK_OK with no launch; TIPK_OK implies correct numbers.
 *   workspace: tipk_distmult_screen_rank_workspace_bytes(n_nodes, dim, n_q, n_tgt) bytes (-1: unsupported).  It is 0 today --
 *   the per-part counts are summed in out_rank itself with integer atomics -- and workspace may then be NULL.
 *   Nothing lives in host memory: the entry does NOT synchronise, may be captured into a hipGraph (two launches) and is
 *   BITWISE repeatable, run to run and route to route (integer counts; no float atomics).
 */
int     tipk_distmult_screen_rank_supported(int64_t n_nodes, int dim, int64_t n_rel);
int64_t tipk_distmult_screen_rank_workspace_bytes(int64_t n_nodes, int dim, int64_t n_q, int64_t n_tgt);   /* -1: unsupported; may be 0 */
int     tipk_distmult_screen_rank_chunk(void);      /* targets of one query ranked per pass (host query; tests read it) */
int     tipk_distmult_screen_rank(const float* z, int64_t n_nodes, int dim, const float* rel_w, int64_t n_rel,
                                  const int32_t* q_rel /* device [n_q] */, int64_t n_q,
                                  const int64_t* tgt_ptr /* device [n_q+1] */,
                                  const int32_t* tgt_u, const int32_t* tgt_v /* device [n_tgt] */, int64_t n_tgt,
                                  const int64_t* known_keys /* nullable */, const int64_t* known_ptr /* [n_rel+1], nullable */,
                                  int32_t* out_rank, float* out_logit /* nullable */, void* workspace, tipk_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * 4i. Add-on burden: the expected weighted number of side effects a CANDIDATE drug brings to a patient's drug list through
 *     its own pairs with that list, per (query, candidate), and the k candidates of every query with the lowest burden
 *     (serving; the prescriptive question after 4e: which drug to add, or which replacement; no reference call site).
 *
 *   Contexts, CSR, DEVICE: ctx_drugs int32 [n_entries], ctx_ptr int64 [n_q + 1].  Context q is the list
 *   ctx_drugs[ctx_ptr[q] .. ctx_ptr[q+1]) of the drugs the patient already takes, in list order.
 *   Candidates, DEVICE: cand int32, cand_ptr int64 [n_q + 1]: query q owns the entries cand[cand_ptr[q] .. cand_ptr[q+1]) and
 *   n_cand is the total number of entries (= cand_ptr[n_q]).  cand_ptr == NULL: the ONE list cand[0 .. n_cand) is shared by
 *   all queries.  A TASK is one (query, candidate entry); the position of a task is its index in its query's list.
 *   weights fp32 [n_rel], nullable (NULL: every weight is 1): finite and >= 0, e.g. a severity per side effect.
 *   Logit of (c, s, r), c the candidate, s a context drug: exactly that of 4d.  DistMult: h_k = z[c,k] * z[s,k] rounded
 *   once, then acc = fmaf(h_k, w[r,k], acc) for k ascending from 0 -- the same bits for (c, s) and (s, c).  Table variant:
 *   the single fp32 add s1[u,r] + s2[v,r] with u = min(c, s), v = max(c, s): what 4e scores for the sorted list S + {c}.
 *   A triple contributes nothing when it is KNOWN: listed for the pair's unordered key in the pair-major lists
 *   (known_pair_keys, known_pair_ptr, known_rel) of 4d, nullable together.
 *   Per task (q, c) and relation r, over the context drugs s of q in list order, chosen by `aggregate` (the constants of 4e):
 *     TIPK_REGIMEN_NOISY_OR  A_r = sum over the contributing triples, in context order, in fp32 (A_r starts at 0.0f and each
 *                            term is added with one rounding), of softplus(s) = fmaxf(s, 0) + log1pf(expf(-fabsf(s))) -- the
 *                            formula of 4e --, and P_r = -expm1f(-A_r): the probability that at least one pair causes r.
 *     TIPK_REGIMEN_MAX       P_r = sigma(L) = 1.0f / (1.0f + expf(-L)), L the largest contributing logit.
 *   A relation with no contributing triple has P_r = 0.
 *   Burden B = sum over r of weights[r] * P_r, an fp32 sum in this fixed order: with l = r mod 64, b_l starts at 0.0f and
 *   takes b_l = fmaf(weights[r], P_r, b_l) for r = l, l + 64, l + 128, ... ascending; then for off = 32, 16, 8, 4, 2, 1:
 *   b_l = b_l + b_(l + off) for l < off; B = b_0.  The order does not depend on the data, the grid, the route or the other
 *   tasks of the call, and the result is BITWISE repeatable.
 *   NOT APPLICABLE -- the burden is NaN, the task is never selected, nothing is read out of bounds: c outside
 *   [0, n_nodes); c occurs in its query's context; a context of 0 or of more than tipk_addon_max_context() (64) entries; a
 *   context that holds an id outside [0, n_nodes); any triple of the task that is not known has a NaN logit (under either
 *   aggregate, whatever the relation's weight); an entry of cand that no query of cand_ptr owns.
 *   Output (device): out_burden fp32, one per task: [n_cand] in the order of cand (cand_ptr given) or [n_q x n_cand] (shared
 *   list).  k > 0: out_best_burden fp32 [n_q x k] and out_best_pos int32 [n_q x k] = the k tasks of each query with the
 *   lowest burden, ascending, ties by ascending position; the selection reads the fp32 values written to out_burden, so the
 *   returned values are bit-equal to out_burden[position]; a row with fewer than k applicable tasks is padded with
 *   (+inf, -1).  k == 0 skips the selection and both pointers may be NULL.
 *   Work: one launch with one wavefront per task (a lane keeps one context drug, lanes own relations as in 4e, the wave
 *   reduces at the end), then, for k > 0, one launch with one wavefront per query on the same stream.
 *   Routes (DistMult): rel_w is staged in LDS once per workgroup when it fits beside the wavefronts' state
 *   (tipk_distmult_addon_burden_lds_route: 1 097 x 16 does); otherwise, or under option "addon_global", every lane reads its
 *   rows from global memory; same bits.
 *   Supported: as 4e -- 1 <= n_nodes <= 46 340, dim % 4 == 0 in 4..256 (DistMult; rel_w 16-byte aligned), 1 <= n_rel <=
 *   65 536, 0 <= k <= 128; at most 2^31 - 1 candidate entries (n_cand).
 *   Status: TIPK_EINVAL -- before anything is launched or written -- for k < 0, a negative size, n_nodes or n_rel < 1,
 *   ld < n_rel, an unknown `aggregate`, a NULL required pointer (ctx_drugs, ctx_ptr, cand, the tables, out_burden, and with
 *   k > 0 the two best outputs; with n_q > 0 and n_cand > 0), known arrays given only in part; then TIPK_EUNSUPPORTED outside
 *   the supported range; n_q == 0 or n_cand == 0 is TIPK_OK with no launch and nothing written; TIPK_OK implies correct
 *   numbers.
 *   workspace: tipk_distmult_addon_burden_workspace_bytes(...) bytes (-1: unsupported); 0 for every supported shape today
 *   and `workspace` may then be NULL.
 *   Nothing lives in host memory: these entries do NOT synchronise and may be captured into a hipGraph (sequential launches,
 *   no parallel branches).
 */
int     tipk_addon_max_context(void);
int     tipk_distmult_addon_burden_supported(int64_t n_nodes, int dim, int64_t n_rel, int k);
int64_t tipk_distmult_addon_burden_workspace_bytes(int64_t n_nodes, int dim, int64_t n_rel, int64_t n_q, int64_t n_cand,
                                                   int k);
int     tipk_distmult_addon_burden_lds_route(int dim, int64_t n_rel);   /* 1 = rel_w is staged in LDS once (options apply) */
int     tipk_distmult_addon_burden(const float* z, int64_t n_nodes, int dim, const float* rel_w, int64_t n_rel,
                                   const int32_t* ctx_drugs, const int64_t* ctx_ptr /* device */, int64_t n_q,
                                   const int32_t* cand, const int64_t* cand_ptr /* device; nullable: shared list */,
                                   int64_t n_cand, const float* weights /* nullable */,
                                   const int64_t* known_pair_keys, const int64_t* known_pair_ptr, const int32_t* known_rel,
                                   int64_t n_known_pairs /* nullable together */,
                                   int aggregate, int k, float* out_burden, float* out_best_burden /* nullable with k == 0 */,
                                   int32_t* out_best_pos /* nullable with k == 0 */, void* workspace, tipk_stream_t stream);
int     tipk_pair_table_addon_burden_supported(int64_t n_nodes, int64_t n_rel, int k);
int     tipk_pair_table_addon_burden(const float* s1, const float* s2, int64_t ld, int64_t n_nodes, int64_t n_rel,
                                     const int32_t* ctx_drugs, const int64_t* ctx_ptr /* device */, int64_t n_q,
                                     const int32_t* cand, const int64_t* cand_ptr /* device; nullable: shared list */,
                                     int64_t n_cand, const float* weights /* nullable */,
                                     const int64_t* known_pair_keys, const int64_t* known_pair_ptr, const int32_t* known_rel,
                                     int64_t n_known_pairs /* nullable together */,
                                     int aggregate, int k, float* out_burden, float* out_best_burden /* nullable with k == 0 */,
                                     int32_t* out_best_pos /* nullable with k == 0 */, tipk_stream_t stream);

/* 4j. Edge attribution of the last R-GCN layer: which recorded interactions of a drug make the model say what it says
 *     (serving; no reference call site -- the identity is that of MyRGCNConv2, src/layers.py:157-188, read backwards).
 *
 *   rgcn2 has no ReLU behind it, so with h [n_nodes x d_in] (row stride ld_h), basis [n_bases x d_in x d_out] dense,
 *   att [n_rel x n_bases] (row stride ld_att), root [d_in x d_out] dense and the in-edges In(v) of node v
 *     z[v] = 1/max(deg_v, 1) * sum_{e in In(v)} h[src_e] W_{rel_e} + h[v] root,      W_r = sum_b att[r,b] basis[b],
 *   and for a probe g [d_out]:  g . z[v] = own + sum_{e in In(v)} c_e.  Both decoders are linear in z[v] with the other drug
 *   held fixed, so a logit splits exactly into one number per recorded interaction of v plus v's own features.
 *   In-edges, CSR, DEVICE: in_ptr int64 [n_nodes + 1], in_src / in_rel int32 [n_edges]: node v owns the positions
 *   in_ptr[v] .. in_ptr[v+1], sorted by (relation, source); deg_v = in_ptr[v+1] - in_ptr[v], duplicates counted (each is an
 *   entry of its own).  Keeping in_src in [0, n_nodes) and in_rel in [0, n_rel) is the caller's contract
 *   (tip_amd.ops.in_edges_by_node guarantees it); in_ptr is clamped to [0, n_edges].
 *   Query q = (node q_node[q], probe row probe[q * ld_probe .. + d_out)), all DEVICE.
 *   Arithmetic, fp32, ONE value per edge on every route -- three nested fma chains, each starting at 0.0f:
 *     G[b,i]  : acc = fmaf(basis[b,i,o], g[o], acc)        for o = 0 .. d_out - 1 ascending
 *     M[s,b]  : acc = fmaf(h[s,i], G[b,i], acc)            for i = 0 .. d_in - 1 ascending
 *     a_e     : acc = fmaf(att[rel_e,b], M[src_e,b], acc)  for b = 0 .. n_bases - 1 ascending
 *     c_e = (1.0f / (float)max(deg_v, 1)) * a_e            (a correctly rounded reciprocal, then one multiply)
 *     own     : R[i]: acc = fmaf(root[i,o], g[o], acc), o ascending; then acc = fmaf(h[v,i], R[i], acc), i ascending.
 *   Output (device), per query: out_contrib fp32 / out_src int32 / out_rel int32 [n_q x k] = the k in-edges of the node with
 *   the largest c_e, c_e descending, ties (+0 and -0 tie) by ascending position in the node's CSR segment, with the edge's
 *   source and relation; a query with fewer than k edges is padded with (-inf, -1, -1); an edge whose c_e is NaN is never
 *   listed.  out_own [n_q] = own.  out_sum [n_q] = the sum of ALL c_e of the node (not only the listed): every fp32 c_e is
 *   added in fp64 -- thread t of 256 adds the edges at positions t, t + 256, ... ascending, lanes are combined by
 *   x_l += x_(l + off) for off = 32, 16, 8, 4, 2, 1, the four wavefronts as ((w0 + w1) + w2) + w3 -- and rounded once to
 *   fp32.  No float atomics anywhere: every output is BITWISE repeatable run to run and route to route.
 *   q_node outside [0, n_nodes): a fully padded row, out_own = out_sum = NaN, nothing read out of bounds.  deg 0: padding
 *   only, out_sum = +0.
 *   Work: ONE launch, one workgroup of 256 threads per query: G, then the table M for every node from h staged through LDS,
 *   then one pass over the node's in-edges with the selection of 4c (LDS buffer, running threshold, bitonic cut).
 *   Routes: M [n_nodes x n_bases] lives in LDS where it fits beside the rest (tipk_rgcn_attribution_lds_route: 645 x 32
 *   does); otherwise, or under option "attribution_global", in `workspace`, one slice per workgroup, and at most 256
 *   workgroups loop over the queries; same code, same bits.
 *   Supported: 1 <= n_nodes <= 46 340, 1 <= n_rel <= 65 536, 1 <= n_bases <= 64, 1 <= d_in, d_out <= 128 (any width),
 *   1 <= k <= 1 024; n_edges and n_q below 2^31.
 *   Status: TIPK_EINVAL -- before anything is launched or written -- for k <= 0, a negative size, n_nodes, n_rel, n_bases,
 *   d_in or d_out < 1, a row stride shorter than its row, a NULL required pointer (with n_q > 0: everything but `workspace`
 *   on the LDS route, and in_src / in_rel when n_edges == 0); then TIPK_EUNSUPPORTED outside the supported range; n_q == 0
 *   is TIPK_OK with no launch and nothing written.
 *   workspace: tipk_rgcn_attribution_workspace_bytes(...) bytes (-1: unsupported); 0 on the LDS route, and `workspace` may
 *   then be NULL.  The value follows the option: ask after setting it.
 *   Nothing lives in host memory: the entry does NOT synchronise or allocate and may be captured into a hipGraph.
 */
int     tipk_rgcn_attribution_supported(int64_t n_nodes, int64_t n_rel, int n_bases, int d_in, int d_out, int k);
int     tipk_rgcn_attribution_lds_route(int64_t n_nodes, int n_bases);          /* 1 = per-query table lives in LDS (options apply) */
int64_t tipk_rgcn_attribution_workspace_bytes(int64_t n_nodes, int n_bases, int64_t n_q);   /* -1 unsupported; may be 0 */
int     tipk_rgcn_attribution(const float* h, int64_t ld_h, int64_t n_nodes, int d_in,
                              const float* basis, const float* att, int64_t ld_att, int64_t n_rel, int n_bases,
                              const float* root, int d_out,
                              const int64_t* in_ptr /* [n_nodes+1] */, const int32_t* in_src, const int32_t* in_rel, int64_t n_edges,
                              const int32_t* q_node /* [n_q] */, const float* probe, int64_t ld_probe, int64_t n_q, int k,
                              float* out_contrib, int32_t* out_src, int32_t* out_rel /* [n_q x k] */,
                              float* out_own, float* out_sum /* [n_q] */, void* workspace, tipk_stream_t stream);

/* 4k. Fold-in: embed drugs that are NOT nodes of the training graph, with the trained model frozen (serving; no reference
 *     call site -- one destination row of MyRGCNConv2, src/layers.py:157-188, twice, behind the P -> D mean of
 *     MyHierarchyConv, src/layers.py:196-247).
 *
 *   A row of an R-GCN layer's output depends on the node's own input row and its in-neighbours' input rows only, so the
 *   embedding of a new drug needs nothing but the tables the encoder already produces: h_prot [n_prot x p] (the P-P encoder's
 *   output, row stride ld_h_prot), x0 [n_nodes x d0] (the mixed drug features, ld_x0) and h1 = relu(rgcn1(x0)) [n_nodes x d1]
 *   (ld_h1); and the parameters hgcn_w [p x pd] dense, basis1 [n_bases x d0 x d1], root1 [d0 x d1], basis2 [n_bases x d1 x
 *   d2], root2 [d1 x d2] dense, att1 / att2 [n_rel x n_bases] (row strides ld_att1 / ld_att2).  d0 = ne + pd with cat != 0,
 *   d0 = ne = pd with cat == 0.
 *   Per new drug m of n_new, all DEVICE: xd [n_new x ne] (ld_xd), its normalised drug-feature embedding (zeros: none);
 *   targets, CSR: tgt_ptr int64 [n_new + 1], tgt_prot int32 [n_tgt] in [0, n_prot); recorded interactions, CSR: in_ptr int64
 *   [n_new + 1], in_src int32 [n_edges] (an EXISTING drug in [0, n_nodes)), in_rel int32 [n_edges] in [0, n_rel): each entry
 *   is one in-edge partner -> new drug; duplicates count.  Keeping the ids in range is the caller's contract
 *   (tip_amd.ops.drug_fold_in checks each tensor once); tgt_ptr and in_ptr are clamped to [0, n_tgt] and [0, n_edges].
 *   With t_m targets and deg_m interactions:
 *     pd_m  = (1/max(t_m,1) * sum_{q in targets} h_prot[q]) hgcn_w
 *     x0_m  = cat(xd_m, pd_m)  |  xd_m + pd_m
 *     h1_m  = relu( 1/max(deg_m,1) * sum_e sum_b att1[rel_e,b] * (x0[src_e] basis1[b]) + x0_m root1 )
 *     z_m   =       1/max(deg_m,1) * sum_e sum_b att2[rel_e,b] * (h1[src_e] basis2[b]) + h1_m root2
 *   -> x0_new [n_new x d0], h1_new [n_new x d1], z_new [n_new x d2] (row strides given).  The existing drugs' rows are held
 *   fixed: the new edges point INTO the new drug only.
 *   Arithmetic, fp32, AGGREGATE FIRST: A1[b,:] = sum_e att1[rel_e,b] * x0[src_e,:] and A2[b,:] = sum_e att2[rel_e,b] *
 *   h1[src_e,:], both in one walk over the segment: per drug this is the product att[rel_e,:]^T [B x deg] . x[src_e,:]
 *   [deg x d] with the edges as K, run on v_mfma_f32_16x16x4_f32 four edges at a time in segment order -- one exact fmaf
 *   chain per entry along the segment, from 0.0f.  Then the contraction [drugs x n_bases d_in] . [n_bases d_in x d_out] on the
 *   same instruction (an exact fmaf chain per output; the K range is dealt to 8 wavefronts in steps of 16 and their partial
 *   sums are added as ((w0+w1)+(w2+w3))+((w4+w5)+(w6+w7))); then one multiply by the correctly rounded
 *   1.0f / (float)max(deg_m, 1), plus the root chain (i ascending, from 0.0f).  The target mean: a chain of adds in segment
 *   order, one multiply by 1.0f / (float)max(t_m, 1), then fmaf over j ascending.
 *   No atomics: every row is BITWISE repeatable and does not depend on which other drugs share the call.
 *   Work: ONE launch, a workgroup of 512 threads per tile of up to 16 new drugs (16 from 4 096 drugs on; fewer per tile in a
 *   smaller call, down to one below 257, so that few drugs with long lists still spread over the chip); each basis is read
 *   once per workgroup; no per-edge or per-drug temporary leaves the chip (LDS images of at most 16 bases at a time; with
 *   more, the segment is walked once per 16 bases).  A long segment is walked by four wavefronts side by side (each owns a
 *   share of the columns) and holds up half of its own tile only.
 *   Supported: 1 <= ne, d0 <= 128; 1 <= p, pd, d1, d2, n_bases <= 64 (any width); 1 <= n_rel <= 2^24; n_nodes, n_prot, n_tgt,
 *   n_edges below 2^31.
 *   Status: TIPK_EINVAL -- before anything is launched or written -- for a negative size, n_nodes, n_prot, n_rel, n_bases or
 *   a width < 1, ne != pd with cat == 0, a row stride shorter than its row, a NULL required pointer (with n_new > 0:
 *   everything but `workspace`, and tgt_prot / in_src / in_rel when their list is empty); then TIPK_EUNSUPPORTED outside the
 *   supported range; n_new == 0 is TIPK_OK with no launch and nothing written.
 *   workspace: tipk_drug_fold_in_workspace_bytes(...) bytes (-1: unsupported); 0 today -- every sum ends inside its
 *   workgroup -- and `workspace` may then be NULL.
 *   Nothing lives in host memory: the entry does NOT synchronise or allocate and may be captured into a hipGraph.
 */
int     tipk_drug_fold_in_supported(int64_t n_nodes, int64_t n_prot, int64_t n_rel, int n_bases, int ne, int p, int pd,
                                    int d1, int d2, int cat);
int64_t tipk_drug_fold_in_workspace_bytes(int64_t n_nodes, int64_t n_prot, int64_t n_rel, int n_bases, int ne, int p, int pd,
                                          int d1, int d2, int cat, int64_t n_new, int64_t n_edges);   /* -1 unsupported; may be 0 */
int     tipk_drug_fold_in(const float* h_prot, int64_t ld_h_prot, int64_t n_prot, int p, const float* hgcn_w, int pd,
                          const float* x0, int64_t ld_x0, const float* h1, int64_t ld_h1, int64_t n_nodes,
                          const float* basis1, const float* att1, int64_t ld_att1, const float* root1,
                          const float* basis2, const float* att2, int64_t ld_att2, const float* root2,
                          int64_t n_rel, int n_bases, int d1, int d2,
                          const float* xd, int64_t ld_xd, int ne, int cat,
                          const int64_t* tgt_ptr /* [n_new+1] */, const int32_t* tgt_prot, int64_t n_tgt,
                          const int64_t* in_ptr /* [n_new+1] */, const int32_t* in_src, const int32_t* in_rel, int64_t n_edges,
                          int64_t n_new, float* x0_new, int64_t ld_x0_new, float* h1_new, int64_t ld_h1_new,
                          float* z_new, int64_t ld_z_new, void* workspace, tipk_stream_t stream);

/* 4l. Partner sum: the expected number of UNRECORDED partners of a drug per side effect -- the marginal of the model over
 *     the partner axis -- and the k side effects of every queried drug with the largest expectation (serving: the
 *     liability profile of one drug, above all of a folded-in compound of 4k; no reference call site).
 *
 *       out_sum[q, j] = sum over the candidates c of  partner_w[c] * sigma(logit(r, u, c)),     u = q_drug[q], r = rel_ids[j]
 *
 *   Input, DEVICE: q_drug int32 [n_q], the queried drugs (entries may repeat); rel_ids int32 [n_sel], nullable: the
 *   relations that are the COLUMNS of the result (entries may repeat); NULL: all relations, column j is relation j, and
 *   n_sel must equal n_rel.  partner_w fp32 [n_nodes], nullable (NULL: every weight is 1), e.g. a co-prescription
 *   frequency; finite and >= 0 is the caller's contract.  known_keys / known_ptr [n_rel + 1]: the relation-major lists of
 *   4c, nullable together.
 *   Candidates of cell (q, j): every drug c in [0, n_nodes) with c != u and partner_w[c] != 0 whose key u*n+c is NOT a key of
 *   relation r.  ONLY THE FORWARD KEY u*n+c is looked up: a caller who wants a recorded pair dropped in both directions
 *   passes lists that hold both directions of every pair (tip_amd.ops.symmetric_known makes them so).
 *   Logits: as 4g.  DistMult: a_k = z[u,k] * w[r,k] rounded once, then acc = fmaf(a_k, z[c,k], acc) for k ascending from 0
 *   -- the queried drug is the one multiplied with w first.  Table variant (tipk_pair_table_partner_sum; the NN decoder of
 *   4b): the RELATION-major tables s1t, s2t [n_rel x ld], ld >= n_nodes; the logit is the single fp32 add
 *   s1t[r,u] + s2t[r,c]: the queried drug is the decoder's first argument.  (The contract of a logit is the per-logit bound
 *   of tests/partner_rank_spec.py, which holds for any order of the dim products; today's kernels give 4g's bits.)
 *   Cell: out_sum fp32 [n_q x n_sel] = the sum over the candidates of partner_w[c] * sigma(logit), sigma(s) =
 *   1.0f / (1.0f + expf(-s)); out_count int32 [n_q x n_sel] = the number of candidates.  Order of the fp32 sum: with
 *   l = c mod 64, p_l starts at +0.0f and takes p_l = p_l + term_c for the candidates c = l, l + 64, ... ascending; then for
 *   off = 32, 16, 8, 4, 2, 1: p_l = p_l + p_(l + off); the cell is p_0.  The order depends on nothing but n_nodes: BITWISE
 *   repeatable, run to run and route to route; no floating-point atomics.
 *   A drug that is no candidate (u itself, weight 0, recorded) is SKIPPED, not multiplied: its logit, NaN or not, does not
 *   reach the sum.  A NaN logit of a candidate makes the cell NaN; a logit of +inf contributes exactly partner_w[c], one of
 *   -inf exactly 0.  A cell without candidates has sum +0 and count 0.
 *   A row whose u is outside [0, n_nodes) and a column whose r is outside [0, n_rel) hold sum NaN and count 0; nothing is
 *   read out of bounds.
 *   Selection, per row (k > 0): out_top_val fp32 [n_q x k], out_top_pos int32 [n_q x k] = the k largest non-NaN cells of the
 *   row, value descending, ties (+0 and -0 tie) by ascending column position; the selection reads the fp32 values written
 *   to out_sum, so the returned values are bit-equal to out_sum at those positions; a row with fewer than k such cells is
 *   padded with (-inf, -1).  k == 0 skips the selection and both pointers may be NULL.
 *   Work: one launch with one wavefront per (queried drug, block of 4 columns): a partner's row is read once and serves the
 *   block's relations (register blocking: the vector ALU is the limit, not LDS); then, for k > 0, one launch with one
 *   wavefront per queried drug on the same stream.
 *   Routes (DistMult): z is staged in LDS once per workgroup when it fits beside the wavefronts' state
 *   (tipk_distmult_partner_sum_lds_route: 645 x 16 does); otherwise, or under option "partner_sum_global", every lane reads
 *   its rows from global memory; same bits.
 *   Supported: as 4g -- 1 <= n_nodes <= 46 340, dim % 4 == 0 in 4..256 (DistMult; z 16-byte aligned),
 *   1 <= n_rel <= 65 536; n_sel below 2^31.
 *   Status: TIPK_EINVAL -- before anything is launched or written -- for k outside 0..128, a negative size, n_nodes or
 *   n_rel < 1, dim < 1, ld < n_nodes, rel_ids == NULL with n_sel != n_rel, a NULL required pointer (q_drug, the tables,
 *   out_sum, out_count, and with k > 0 the two top outputs; with n_q > 0 and n_sel > 0), keys without offsets or the
 *   reverse; then TIPK_EUNSUPPORTED outside the supported range; n_q == 0 or n_sel == 0 is TIPK_OK with no launch and
 *   nothing written; TIPK_OK implies correct numbers.
 *   No workspace.  Nothing lives in host memory: these entries do NOT synchronise and may be captured into a hipGraph
 *   (sequential launches, no parallel branches).
 */
int     tipk_distmult_partner_sum_supported(int64_t n_nodes, int dim, int64_t n_rel);
int     tipk_distmult_partner_sum_lds_route(int64_t n_nodes, int dim);   /* 1 = z is staged in LDS once (options apply) */
int     tipk_distmult_partner_sum(const float* z, int64_t n_nodes, int dim, const float* rel_w, int64_t n_rel,
                                  const int32_t* q_drug /* device */, int64_t n_q,
                                  const int32_t* rel_ids /* device; nullable: all relations */, int64_t n_sel,
                                  const float* partner_w /* nullable */,
                                  const int64_t* known_keys /* nullable */, const int64_t* known_ptr /* [n_rel+1], nullable */,
                                  int k, float* out_sum, int32_t* out_count, float* out_top_val /* nullable with k == 0 */,
                                  int32_t* out_top_pos /* nullable with k == 0 */, tipk_stream_t stream);
int     tipk_pair_table_partner_sum_supported(int64_t n_nodes, int64_t n_rel);
int     tipk_pair_table_partner_sum(const float* s1t, const float* s2t, int64_t ld, int64_t n_nodes, int64_t n_rel,
                                    const int32_t* q_drug /* device */, int64_t n_q,
                                    const int32_t* rel_ids /* device; nullable: all relations */, int64_t n_sel,
                                    const float* partner_w /* nullable */,
                                    const int64_t* known_keys /* nullable */, const int64_t* known_ptr /* [n_rel+1], nullable */,
                                    int k, float* out_sum, int32_t* out_count, float* out_top_val /* nullable with k == 0 */,
                                    int32_t* out_top_pos /* nullable with k == 0 */, tipk_stream_t stream);

/* 4m. Fit of decoder rows for NEW side effects with the trained model frozen (serving; no reference call site): the
 *     missing row of the DistMult decoder of 4a for a side effect the model was not trained on, from its recorded pairs.
 *
 *   Objective of new side effect b with row w, s(u,v) = sum_k z[u,k] z[v,k] w[k] -- the expectation of the training
 *   objective over its one uniform negative per positive (tip_amd/neg_sampling.py), with the exact softplus:
 *     L_b(w) = sum_{distinct recorded p} wpos_p softplus(-s_p)
 *            + dense_w[b] * sum_{ordered (u,v) in [0,n)^2 NOT recorded} softplus(s)  +  l2/2 |w|^2
 *   evaluated as  dense_w[b] * sum over ALL unordered u <= v of m softplus(s), m = 2 (1 for u == v)  -- a mask-free stream --
 *   plus, per distinct recorded unordered pair, wpos_p softplus(-s_p) - wneg_p softplus(s_p): wpos = multiplicity / P_b,
 *   wneg = dense_w[b] * (ordered multiplicity 2 | 1), dense_w[b] = neg_weight / N_b (tip_amd.ops.fit_pairs_csr builds them).
 *
 *   tipk_distmult_fit_stats.  Input, DEVICE: z [n_nodes x dim] dense, 16-byte aligned; the trial rows w [n_fit x dim];
 *   dense_w fp32 [n_fit]; the distinct recorded pairs as CSR: pair_ptr int64 [n_fit + 1], pair_u / pair_v int32 [n_pairs] in
 *   [0, n_nodes) (the caller's contract; an id outside is clamped, nothing is read out of bounds), pair_wpos / pair_wneg
 *   fp32 [n_pairs]; l2 >= 0; active int32 [n_fit], nullable (NULL: every relation).  Output: loss [n_fit], grad
 *   [n_fit x dim], hess [n_fit x dim x dim] (row-major, both triangles), the l2 terms included.  Rows of an inactive
 *   relation are NOT touched.
 *   Arithmetic, fp32.  Feature f_k = z[u,k] * z[v,k] rounded once; logit: acc = fmaf(f_k, w[k], acc), k ascending from
 *   +0.0f; e = expf(-|s|), r = 1.0f / (1.0f + e): softplus(s) = fmaxf(s, 0) + log1pf(e), sigma(s) = r (s >= 0) | e r,
 *   sigma'(s) = e r r.  Terms: loss c softplus, gradient c sigma f_i, Hessian c sigma' f_i f_j with c = m dense_w[b].
 *   Summation order.  Tiles of 64 x 64 pairs (u-block, v-block >= u-block) are numbered u-block major; the tiles are cut
 *   into tipk_distmult_fit_slabs(n_nodes, dim, n_fit) SLABS of equal length (the last may be shorter).  In a tile wavefront
 *   q of 4 owns the rows u = 16 q .. 16 q + 15, in ascending order; within a row the gradient and Hessian entries take the
 *   64 pairs in v order on v_mfma_f32_16x16x4_f32 with the pairs as K (an exact fmaf chain), the loss lane v adds its own
 *   term and the 64 lanes are summed at the end of the slab by the halving tree.  One accumulator per (slab, wavefront)
 *   runs through the slab: at most 1 024 terms per tile.  Then, per output, the 4 * slabs partials are added in ascending
 *   (slab, wavefront) order from +0.0f; the recorded pairs are summed in chunks of 256 (a chain from +0.0f in list order,
 *   the chunk totals added in ascending order from +0.0f); result = dense + sparse, then + l2 term (loss: l2/2 times the
 *   fmaf chain of w_k^2; gradient: + l2 w_i; Hessian diagonal: + l2).
 *   tipk_distmult_fit_max_chain(n_nodes, dim, n_fit) = D, the largest number of fp32 additions a term passes through:
 *     max(1 024 * tiles per slab + 6 + 4 * slabs,  256 + ceil(n (n + 1) / 2 / 256)) + 2.
 *   Slabs and D depend on (n_nodes, dim, n_fit) alone.  No floating-point atomics, no workgroup waits for another: the
 *   results are BITWISE repeatable call to call.
 *   A NaN logit makes every statistic of ITS relation NaN and touches no other relation (a NaN row of z reaches every
 *   relation; a NaN in one trial row only that relation).
 *   An INFINITE z[u,k] (no NaN logit; w[k] != 0, the other entries of column k != 0) gives logits of +-inf on row u: for
 *   every relation that sees the row -- dense_w[b] > 0, or a recorded pair on u -- grad[k] and row k and column k of hess
 *   are non-finite (+inf or NaN: sigma' = 0 meets an infinite feature), so tipk_newton_step ends that relation with
 *   status 3; the loss is +inf or NaN as soon as one unrecorded pair has the logit +inf or one recorded pair -inf; every
 *   other entry of grad and hess stays finite.  Nothing finite is invented.
 *   Work: a dense launch of slabs x ceil(n_fit / 4) workgroups -- the feature of a pair is computed once for the 4 relations
 *   of the block; both row blocks of a tile are staged in LDS (rows 16-byte aligned, stride width + 4 floats) -- then a
 *   finishing launch of one workgroup per relation.  A workgroup whose relations are all inactive returns at once.
 *   workspace: tipk_distmult_fit_workspace_bytes(n_nodes, dim, n_fit) bytes (-1: unsupported; n_fit == 0: 0), which also
 *   holds the state of tipk_distmult_fit; the statistics entry uses its head.
 *
 *   tipk_newton_step.  One wavefront per relation; all state in caller-provided DEVICE arrays: the accepted row w
 *   [n_fit x dim], its loss [n_fit] and grad [n_fit x dim], the direction p [n_fit x dim], the step t [n_fit], info int32
 *   [n_fit x 4] = (status, evaluations, accepted, rejected), the trial row w_trial [n_fit x dim] and active int32 [n_fit].
 *   Before the first call: info = 0, t = 1, w = w_trial = the start.  Given the statistics at w_trial:
 *     a relation whose status is not 0: active = 0, nothing else.
 *     evaluations == 0:  the trial is taken as accepted (it is the start).
 *     else accept iff  loss_trial <= loss + 1e-4f * t * (g . p) + 16 * 2^-24 * |loss|   (g . p: xor-butterfly sum).
 *     accepted: (w, loss, grad) <- trial;  p <- -H^-1 g by Cholesky (column order; a pivot that is not > 0, or not finite:
 *               p <- -g / max_i H_ii, or -g when that maximum is not > 0);  t <- 1.     rejected: t <- t / 2.
 *     a non-finite statistic: status 3; the accepted row is kept and the trial counts as rejected (at the first call the
 *               trial is the start: it is kept and nothing is counted).
 *     then status 1 if max_i |grad_i| <= gtol, else 2 if t < 2^-20, else 0; evaluations += 1.
 *     status 0: w_trial <- fmaf(t, p, w) and active = 1; otherwise active = 0.
 *   evaluations = accepted + rejected + 1 at all times after the first call.
 *
 *   tipk_distmult_fit.  Enqueues one initialising launch (start = init [n_fit x dim], NULL: zeros) and max_iter + 1
 *   (statistics, step) pairs on `stream`; the active mask makes a finished relation's workgroups return at once.  Output:
 *   out_w [n_fit x dim], out_loss [n_fit], out_grad [n_fit x dim] = the accepted row and its statistics, out_info int32
 *   [n_fit x 4] as above (status 0 after max_iter + 1 evaluations: not converged).
 *   Supported: 1 <= n_nodes <= 46 340, dim % 4 == 0 in 4..32 (widths below 16 | 32 zero-padded on chip), 1 <= n_fit <=
 *   65 536; z 16-byte aligned.
 *   Status: TIPK_EINVAL -- before anything is launched or written -- for a negative size, n_nodes or dim < 1, l2 < 0 or NaN,
 *   gtol < 0 or NaN, max_iter < 0, a NULL required pointer (with n_fit > 0: everything but `active`, `init` and, with
 *   n_pairs == 0, the four pair arrays); then TIPK_EUNSUPPORTED outside the supported range; n_fit == 0 is TIPK_OK with no
 *   launch and nothing written.
 *   Nothing lives in host memory: the entries do NOT synchronise or allocate and may be captured into a hipGraph
 *   (sequential launches, no parallel branches).
 */
int     tipk_distmult_fit_supported(int64_t n_nodes, int dim, int64_t n_fit);
int64_t tipk_distmult_fit_slabs(int64_t n_nodes, int dim, int64_t n_fit);            /* -1 unsupported */
int64_t tipk_distmult_fit_max_chain(int64_t n_nodes, int dim, int64_t n_fit);        /* -1 unsupported */
int64_t tipk_distmult_fit_workspace_bytes(int64_t n_nodes, int dim, int64_t n_fit);  /* -1 unsupported */
int     tipk_distmult_fit_stats(const float* z, int64_t n_nodes, int dim, const float* w, int64_t n_fit,
                                const float* dense_w, const int64_t* pair_ptr /* [n_fit+1] */, const int32_t* pair_u,
                                const int32_t* pair_v, const float* pair_wpos, const float* pair_wneg, int64_t n_pairs,
                                float l2, const int32_t* active /* nullable */, float* loss, float* grad, float* hess,
                                void* workspace, tipk_stream_t stream);
int     tipk_newton_step(int dim, int64_t n_fit, const float* stat_loss, const float* stat_grad, const float* stat_hess,
                         float gtol, float* w, float* loss, float* grad, float* p, float* t, int32_t* info,
                         float* w_trial, int32_t* active, tipk_stream_t stream);
int     tipk_distmult_fit(const float* z, int64_t n_nodes, int dim, int64_t n_fit, const float* dense_w,
                          const int64_t* pair_ptr /* [n_fit+1] */, const int32_t* pair_u, const int32_t* pair_v,
                          const float* pair_wpos, const float* pair_wneg, int64_t n_pairs, float l2,
                          const float* init /* nullable: zeros */, int max_iter, float gtol,
                          float* out_w, float* out_loss, float* out_grad, int32_t* out_info, void* workspace,
                          tipk_stream_t stream);

/* 4n. Combination burden: the TOTAL expected weighted number of side effects of every regimen a query can form by choosing
 *     one alternative per open slot on top of its fixed drugs, per (query, combination), and the k combinations of every
 *     query with the lowest burden (serving; the question after 4i when more than one choice is open: which trio of
 *     alternatives, which drugs of a list to stop; no reference call site).
 *
 *   A QUERY q is a list of FIXED drugs (possibly empty) and S >= 0 SLOTS, each a non-empty list of ALTERNATIVES: a drug id, or
 *   -1 for "leave this slot empty".  All lists are DEVICE arrays:
 *     fix_drugs int32 [n_fix], fix_ptr int64 [n_q + 1]: the fixed drugs of q, in list order;
 *     slot_ptr int64 [n_q + 1]: q owns the slots slot_ptr[q] .. slot_ptr[q+1]; alt_ptr int64 [n_slots + 1], alt int32 [n_alt]:
 *     slot s owns alt[alt_ptr[s] .. alt_ptr[s+1]).  A_s is the size of slot s; the alternatives of q are numbered j = 0, 1, ...
 *     in slot order.
 *   A COMBINATION picks one alternative per slot; its index is c = sum_s c_s * prod_{t > s} A_t: the LAST slot runs fastest
 *   (itertools.product).  A query has C = prod_s A_s combinations (1 with S = 0: the fixed list alone).
 *     comb_ptr int64 [n_q + 1]: q owns out_burden[comb_ptr[q] - comb_ptr[0] .. comb_ptr[q+1] - comb_ptr[0]); n_comb is the
 *     number of entries of the call.  row_ptr int64 [n_q + 1]: q owns that range of workspace rows (relative to row_ptr[0]);
 *     a legal query has 1 + sum_s A_s + sum_{s < t} A_s A_t of them and n_rows is the total.  Both are taken relative to
 *     their first entry, so a caller may pass a window [q0, q1] of longer arrays.
 *   The REGIMEN of a combination is the fixed drugs plus the chosen ids that are not -1.  Its burden follows 4d / 4i: for
 *   every unordered pair of the regimen the logit is that of the pair (min id, max id) -- 4i's arithmetic, DistMult or
 *   table --, and a triple contributes unless it is KNOWN for the pair's key (the pair-major lists of 4d).  Per relation r
 *     TIPK_REGIMEN_NOISY_OR  A_r = sum of softplus(logit) over the contributing triples, P_r = -expm1f(-A_r)
 *     TIPK_REGIMEN_MAX       P_r = sigma(L) = 1.0f / (1.0f + expf(-L)), L the largest contributing logit
 *   P_r = 0 without a contributing triple; B = sum_r weights[r] * P_r.  A regimen of 0 or 1 drugs has B = +0 exactly.
 *   ORDER of the fp32 sums (noisy-or), fixed and the same on every route -- LEVEL ORDER.  Three kinds of partial sums, each a
 *   chain of one-rounding adds from +0.0f:
 *     base_r       over the pairs (i, j), i < j, of the fixed list, i ascending, then j ascending;
 *     single[j]_r  alternative j with the fixed drugs in list order;
 *     cross[j][j']_r  the one term of the pair of alternatives j, j' of different slots.
 *   A_r = base_r; then for s = 1 .. S: A_r += single[c_s]_r, then A_r += cross[c_s][c_t]_r for t = 1 .. s - 1 ascending; the
 *   terms of a -1 alternative are skipped (not added as zeros).  Under TIPK_REGIMEN_MAX the same terms hold largest logits
 *   (-inf: none) and the sum is a maximum.  Then the sum over r as 4i: with l = r mod 64, b_l = fmaf(weights[r], P_r, b_l)
 *   for r = l, l + 64, ... ascending from 0.0f, then b_l = b_l + b_(l + off) for off = 32, 16, 8, 4, 2, 1; B = b_0.  The order
 *   depends on nothing but the query: BITWISE repeatable, run to run and route to route; no floating-point atomics.
 *   NOT APPLICABLE -- the burden is NaN and the combination is never selected: two chosen drugs coincide; a chosen drug is
 *   a fixed drug; any triple of its pairs that is not known has a NaN logit (under either aggregate, whatever the weights).
 *   ILLEGAL QUERY -- every entry of its comb_ptr range is NaN and nothing is read out of bounds: a fixed id outside
 *   [0, n_nodes); a repeated fixed drug; an alternative outside [-1, n_nodes); an empty slot; more than
 *   tipk_addon_max_context() (64) fixed drugs, tipk_combo_max_slots() (10) slots, tipk_combo_max_alternatives() (64)
 *   alternatives in all its slots or tipk_combo_max_combinations() (2^24) combinations; offsets that leave [0, n_fix],
 *   [0, n_slots], [0, n_alt], [0, n_comb] or [0, n_rows] or descend; a comb_ptr range that is not C entries or a row_ptr range
 *   that is not the row count above.  An entry of out_burden that no query owns is NaN.
 *   Output (device): out_burden fp32 [n_comb].  k > 0: out_best_burden fp32 [n_q x k], out_best_comb int32 [n_q x k] = the k
 *   combinations of each query with the lowest burden, ascending, ties by ascending combination index; the selection reads
 *   the fp32 values written to out_burden; padding is (+inf, -1).  k == 0 skips the selection and both may be NULL.
 *   Work: three launches on one stream.  (1) Tables: one wavefront per (query, row) -- base, single[j], cross[j][j'] -- with
 *   lane-owned relations in windows as 4i; a row of n_rel floats goes to `workspace` (row stride n_rel rounded up to 4
 *   floats) with coalesced stores; a NaN logit of a triple that is not known is stored as NaN and wins every maximum, and
 *   the row of a pair that cannot be (one drug twice, an alternative that is fixed) is NaN throughout.  (2) Burden:
 *   persistent workgroups, a wavefront takes runs of consecutive combinations and reads its rows from the workspace; while
 *   only the last slot advances the sum through level S - 1 is kept per relation in LDS (n_rel <= 2 048; option
 *   "combo_no_prefix" turns it off, "combo_run" sets the run length): same bits.  (3) Selection, one wavefront per query.
 *   Supported: as 4i -- 1 <= n_nodes <= 46 340, dim % 4 == 0 in 4..256 (DistMult; rel_w 16-byte aligned), 1 <= n_rel <=
 *   65 536, 0 <= k <= 128; n_comb below 2^31; workspace 16-byte aligned.
 *   Status: TIPK_EINVAL -- before anything is launched or written -- for k < 0, a negative size, n_nodes or n_rel < 1,
 *   ld < n_rel, an unknown `aggregate`, a NULL required pointer (with n_q > 0: the five offset arrays, the tables, fix_drugs
 *   with n_fix > 0, alt with n_alt > 0, out_burden with n_comb > 0, workspace with n_rows > 0, and with k > 0 the two best
 *   outputs), known arrays given only in part; then TIPK_EUNSUPPORTED outside the supported range; n_q == 0 is TIPK_OK with no
 *   launch and nothing written; TIPK_OK implies correct numbers.
 *   workspace: tipk_*_combo_burden_workspace_bytes(..., n_rows, k) bytes (-1: unsupported; may be 0).
 *   Nothing lives in host memory: these entries do NOT synchronise or allocate and may be captured into a hipGraph
 *   (sequential launches, no parallel branches).
 */
int     tipk_combo_max_slots(void);
int     tipk_combo_max_alternatives(void);
int64_t tipk_combo_max_combinations(void);
int     tipk_distmult_combo_burden_supported(int64_t n_nodes, int dim, int64_t n_rel, int k);
int64_t tipk_distmult_combo_burden_workspace_bytes(int64_t n_nodes, int dim, int64_t n_rel, int64_t n_rows, int k);
int     tipk_distmult_combo_burden(const float* z, int64_t n_nodes, int dim, const float* rel_w, int64_t n_rel,
                                   const int32_t* fix_drugs, const int64_t* fix_ptr /* device [n_q+1] */, int64_t n_fix,
                                   const int32_t* alt, const int64_t* alt_ptr /* device [n_slots+1] */, int64_t n_alt,
                                   const int64_t* slot_ptr /* device [n_q+1] */, int64_t n_slots,
                                   const int64_t* comb_ptr, const int64_t* row_ptr /* device [n_q+1] */, int64_t n_q,
                                   int64_t n_comb, int64_t n_rows, const float* weights /* nullable */,
                                   const int64_t* known_pair_keys, const int64_t* known_pair_ptr, const int32_t* known_rel,
                                   int64_t n_known_pairs /* nullable together */,
                                   int aggregate, int k, float* out_burden, float* out_best_burden /* nullable with k == 0 */,
                                   int32_t* out_best_comb /* nullable with k == 0 */, void* workspace, tipk_stream_t stream);
int     tipk_pair_table_combo_burden_supported(int64_t n_nodes, int64_t n_rel, int k);
int64_t tipk_pair_table_combo_burden_workspace_bytes(int64_t n_nodes, int64_t n_rel, int64_t n_rows, int k);
int     tipk_pair_table_combo_burden(const float* s1, const float* s2, int64_t ld, int64_t n_nodes, int64_t n_rel,
                                     const int32_t* fix_drugs, const int64_t* fix_ptr /* device [n_q+1] */, int64_t n_fix,
                                     const int32_t* alt, const int64_t* alt_ptr /* device [n_slots+1] */, int64_t n_alt,
                                     const int64_t* slot_ptr /* device [n_q+1] */, int64_t n_slots,
                                     const int64_t* comb_ptr, const int64_t* row_ptr /* device [n_q+1] */, int64_t n_q,
                                     int64_t n_comb, int64_t n_rows, const float* weights /* nullable */,
                                     const int64_t* known_pair_keys, const int64_t* known_pair_ptr, const int32_t* known_rel,
                                     int64_t n_known_pairs /* nullable together */,
                                     int aggregate, int k, float* out_burden, float* out_best_burden /* nullable with k == 0 */,
                                     int32_t* out_best_comb /* nullable with k == 0 */, void* workspace, tipk_stream_t stream);

/* 4o. Protein attribution: which protein targets -- of the explained drug AND of the drugs it interacts with -- a prediction
 *     rests on (serving; no reference call site -- FMEncoder.forward, src/layers.py:520-550, read backwards).
 *
 *   Both R-GCN layers are bias-free, the only non-linearity between the drug inputs and z is the ReLU behind rgcn1, and the
 *   P -> D stage is linear in the protein embeddings.  For the ReLU pattern of the stored h, probe . z[v] therefore equals
 *   gradient x input summed over every protein and every drug's own feature row: an exact partition of the logit.
 *   Operands (DEVICE, fp32): hp [n_prot x p] (ld_hp) the P-P encoder's output by protein id; w_pd [p x pd] dense;
 *   xe [n_nodes x ne] (ld_xe) the drug embedding rows already divided by d_norm; h [n_nodes x d1] (ld_h) the stored
 *   relu(rgcn1(x0)), read ONLY for the mask h > 0; layer l = basis_l dense, att_l [n_rel x n_bases] (ld_att_l), root_l dense:
 *   basis1 [n_bases x d0 x d1], root1 [d0 x d1], basis2 [n_bases x d1 x d2], root2 [d1 x d2], d0 = cat ? ne + pd : ne
 *   (add: ne == pd).
 *   D-D in-edges, CSR by destination: pe_ptr int64 [n_nodes + 1], pe_src / pe_rel int32 [n_edges]; node j owns the positions
 *   pe_ptr[j] .. pe_ptr[j+1], sorted by (SOURCE, relation) (tip_amd.ops.in_edges_by_pair) -- the edges of one pair are
 *   adjacent and in the order they have in the (relation, source) segment of 4j; deg_j = max(pe_ptr[j+1] - pe_ptr[j], 1),
 *   duplicates counted, a self pair is an edge like any other.
 *   Protein-side CSR of the P -> D edges: prot_ptr int64 [n_prot + 1], prot_drug int32 [n_pd_edges] (the drugs protein t
 *   targets, duplicates kept), inv_cnt fp32 [n_nodes] = the correctly rounded 1.0f / max(number of P -> D edges into the
 *   drug, 1).  Ids in range are the caller's contract (tip_amd.ops checks them once per tensor); an id out of range is
 *   skipped, the pointers are clamped, nothing is read out of bounds.
 *   Query q = (node v = q_node[q], probe g = probe[q * ld_probe .. + d2)).
 *   Arithmetic, fp32, every chain starts at 0.0f and runs ascending:
 *     cells    C_l[i,j,b] = (1.0f / deg_j) * (sum of att_l[rel_e, b] over the edges e: i -> j, by plain adds)    (once per call)
 *     G2[b,i]  fma over o of basis2[b,i,o] g[o];   R2[i] fma over o of root2[i,o] g[o]
 *     a1[j,i]  (fma over b of C2[j,v,b] G2[b,i], then + R2[i] where j == v) where h[j,i] > 0, else 0
 *     U[i,b,o] sum over j of C1[i,j,b] a1[j,o] on v_mfma_f32_32x32x2_f32 (exact fp32, j ascending)
 *     a0[i,c]  ONE fma chain: basis1[b,c,o] U[i,b,o] over (b, o), then root1[c,o] a1[i,o] over o
 *     own_i    fma over c < ne of a0[i,c] xe[i,c];   qv[i,x] fma over c < pd of w_pd[x,c] a0[i, (cat ? ne : 0) + c]
 *     c_t      plain adds, over t's entries e ascending, of inv_cnt[i_e] * (fma over x of hp[t,x] qv[i_e,x])
 *     direct_t the same sum over the entries with i_e == v only.
 *   Candidates: the proteins with at least one entry.  Output (device), per query: out_contrib fp32 / out_protein int32 /
 *   out_direct fp32 [n_q x k] = the k candidates with the largest c_t, c_t descending, ties (+0 and -0 tie) by ascending
 *   protein id, with direct_t; fewer than k candidates are padded with (-inf, -1, +0); a NaN c_t is never listed.
 *   out_features [n_q] = sum_i own_i, out_proteins [n_q] = the sum of c_t over ALL candidates: fp32 values added in fp64 --
 *   thread t of 256 adds the items t, t + 256, ... ascending, lanes by x_l += x_(l + off), off = 32 .. 1, the four wavefronts
 *   as ((w0 + w1) + w2) + w3 -- and rounded once.  Then g . z[v] = out_features + out_proteins up to rounding.
 *   No float atomics: every output is BITWISE repeatable, and the same for a query whatever else is in the call.
 *   q_node outside [0, n_nodes): a fully padded row, out_features = out_proteins = NaN, nothing read out of bounds.
 *   Work: the cells kernel once; then per chunk of tipk_protein_attribution_chunk() = 256 queries three launches (a1; the
 *   large product with everything behind it -- a workgroup owns a drug i and 256 / d1p columns' worth of queries, C1[i] and
 *   a1 stream through LDS in slices of 32 rows, U and a0 never leave the chip --; the protein pass with the selection of 4c).
 *   Queries beyond one chunk are looped inside the entry.
 *   Supported: 1 <= n_nodes <= 4 096 (the dense cells take 2 n_nodes^2 n_bases floats), 1 <= n_bases <= 64, every width
 *   (p, pd, ne, d0, d1, d2) in [1, 128] and any value, 1 <= k <= 1 024; n_prot, n_rel, n_edges, n_pd_edges, n_q below 2^31.
 *   Status: TIPK_EINVAL -- before anything is launched or written -- for k <= 0, a negative size, a size or width < 1, a row
 *   stride shorter than its row, add mode with ne != pd, a NULL required pointer (with n_q > 0: everything, `workspace`
 *   included, but pe_src / pe_rel when n_edges == 0 and prot_drug when n_pd_edges == 0); then TIPK_EUNSUPPORTED outside the
 *   supported range; n_q == 0 is TIPK_OK with no launch and nothing written.
 *   workspace: tipk_protein_attribution_workspace_bytes(...) bytes (-1: unsupported sizes), 4-byte aligned.
 *   Nothing lives in host memory: the entry does NOT synchronise or allocate and may be captured into a hipGraph.
 */
int     tipk_protein_attribution_supported(int64_t n_nodes, int64_t n_prot, int64_t n_rel, int n_bases, int ne, int pd, int p,
                                           int d1, int d2, int cat, int k);
int64_t tipk_protein_attribution_chunk(void);
int64_t tipk_protein_attribution_workspace_bytes(int64_t n_nodes, int n_bases, int d1, int p, int64_t n_q);   /* -1 unsupported */
int     tipk_protein_attribution(const float* hp, int64_t ld_hp, int64_t n_prot, int p, const float* w_pd, int pd,
                                 const float* xe, int64_t ld_xe, int ne, const float* h, int64_t ld_h, int64_t n_nodes, int d1,
                                 const float* basis1, const float* att1, int64_t ld_att1, const float* root1,
                                 const float* basis2, const float* att2, int64_t ld_att2, const float* root2, int d2,
                                 int64_t n_rel, int n_bases,
                                 const int64_t* pe_ptr /* [n_nodes+1] */, const int32_t* pe_src, const int32_t* pe_rel, int64_t n_edges,
                                 const int64_t* prot_ptr /* [n_prot+1] */, const int32_t* prot_drug, int64_t n_pd_edges,
                                 const float* inv_cnt /* [n_nodes] */, int cat,
                                 const int32_t* q_node /* [n_q] */, const float* probe, int64_t ld_probe, int64_t n_q, int k,
                                 float* out_contrib, int32_t* out_protein, float* out_direct /* [n_q x k] */,
                                 float* out_features, float* out_proteins /* [n_q] */, void* workspace, tipk_stream_t stream);

/* 4p. Confidence of a side-effect prediction (serving; no reference call site): a Gaussian (Laplace) posterior of DistMult
 *     decoder rows from the Hessian of 4m, and the pair top-k of 4d ranked on a key that knows the variance of every logit.
 *
 *   Model (a modelling choice).  Row b has the Hessian H_b of 4m at w_b (l2 > 0: positive definite)
 *   and P_b recorded pairs; its posterior is N(w_b, (P_b H_b)^-1), the embeddings taken as exact.  With H_b = L_b L_b^T and
 *   W_b = P_b^(-1/2) L_b^-1 (lower triangular) the logit s = phi . w_b of the feature phi = z[u] * z[v] has the variance
 *   var = |W_b phi|^2.
 *
 *   tipk_spd_factor.  DEVICE: hess fp32 [n_rows x dim x dim] row-major, of which ONLY the lower triangle (column <= row) is
 *   read; row_scale fp32 [n_rows] (P_b^(-1/2), the caller's).  Output: out_l [n_rows x dim x dim] row-major, L_b =
 *   chol(H_b); out_w [n_rows x dim x dim] = W_b = row_scale[b] L_b^-1 stored TRANSPOSED: W_b[i][j] is at
 *   out_w[(b * dim + j) * dim + i] -- the 4 columns x 16 rows a lane group of the query's matrix-core operand reads are 64
 *   consecutive floats; status int32 [n_rows], 1 = factored.  The strict upper triangles of L_b and W_b (j > i) are exact
 *   +0.0f.  A row with a pivot that is not > 0 or not finite, a non-finite entry in its lower triangle or a non-finite
 *   row_scale has status 0 and L_b = W_b = 0 throughout; no other row is affected.
 *   Arithmetic, fp32, one wavefront per row: the right-looking Cholesky of tipk_newton_step (4m; the same loop): column k
 *   takes d = sqrtf(pivot), L[i][k] = L[i][k] / d for i > k, then L[i][c] = fmaf(-L[i][k], L[c][k], L[i][c]) for
 *   k < c <= i.  Column c of W_b by forward substitution of row_scale[b] e_c: x_k = x_k / L[k][k], then
 *   x_i = fmaf(-L[i][k], x_k, x_i) for i > k, k ascending from c.  BITWISE repeatable; a row's bits depend on that row alone.
 *   Supported: 1 <= dim <= 32, n_rows < 2^31.  Status: TIPK_EINVAL for a negative n_rows, dim < 1, a NULL pointer (with
 *   n_rows > 0); then TIPK_EUNSUPPORTED; n_rows == 0 is TIPK_OK with no launch.
 *
 *   tipk_distmult_pair_conf_topk.  z [n_nodes x dim], rel_w [n_rel x dim], w_fac [n_rel x dim x dim] = the out_w of
 *   tipk_spd_factor for the same rows; pair_u / pair_v and the pair-major known lists exactly as in 4d.
 *   Arithmetic, fp32, per (pair, relation r): phi_j = z[u,j] * z[v,j] rounded once; the logit s and every
 *   y_i = sum_j W_r[i][j] phi_j are fmaf chains over ALL j < dim ascending from +0.0f (v_mfma_f32_16x16x4_f32 is that chain;
 *   the zeros of the upper triangle are multiplied, so an infinite phi_j gives NaN); the rows are dealt to four groups,
 *   group g owning i = 16 h + 4 g + x (h = 0, 1; x = 0..3; rows >= dim count as y_i = 0): t_g = the chain
 *   fmaf(y_i, y_i, t_g) from +0.0f with h then x ascending, and var = (t_0 + t_1) + (t_2 + t_3).
 *   Key: mode TIPK_CONF_MODERATED (0): s / sqrtf(fmaf(pi/8, var, 1.0f)), pi/8 = 0.39269908169872414f -- the logit of
 *   MacKay's moderated probability; mode TIPK_CONF_BOUND (1): fmaf(c, sqrtf(var), s), c finite (c < 0 a lower bound of the
 *   logit, c > 0 an upper one, c == 0 the logit itself); sqrtf and the division correctly rounded.
 *   Output per pair (device), each [n_pairs x k]: out_key fp32, out_rel int32, out_logit fp32, out_var fp32 = the k relations
 *   with the largest key among those not known for the pair, key descending, ties by ascending relation id; a row with fewer
 *   than k candidates -- and the whole row of a pair with an id outside [0, n_nodes) -- is padded with (-inf, -1, -inf, +inf).
 *   A NaN key is never returned.  dense_logit / dense_var fp32 [n_pairs x n_rel] (nullable together): s and var of EVERY
 *   relation, known ones included; (-inf, +inf) throughout for a pair with an id out of range.  The top-k bits are the same
 *   with and without the dense outputs.  No [n_pairs x n_rel x dim] temporary, no float atomics: BITWISE repeatable, a
 *   pair's bits the same whatever else is in the call.
 *   Work: persistent workgroups of 16 wavefronts, one per CU; a workgroup takes 16 pairs (the N of the matrix-core tile,
 *   their phi resting in registers) through all relations in tiles of 256, wavefront w scoring 16 relations of the tile with
 *   w_fac read straight from L2; then wavefront p selects for pair p from the tile in LDS.
 *   Supported: 1 <= n_nodes <= 46 340, dim % 4 == 0 in 4..32, 1 <= n_rel <= 65 536, 0 <= k <= 128 (k == 0: the dense
 *   outputs only; the four top-k pointers may be NULL).
 *   Status: TIPK_EINVAL -- before anything is launched or written -- for k < 0, a negative size, n_nodes, n_rel or dim < 1,
 *   a mode that is not 0 or 1, c not finite, a NULL required pointer (with n_pairs > 0), known arrays or dense outputs given
 *   only in part; then TIPK_EUNSUPPORTED outside the supported range; n_pairs == 0 is TIPK_OK with no launch.
 *   Nothing lives in host memory: the entries do NOT synchronise or allocate and may be captured into a hipGraph.
 */
#define TIPK_CONF_MODERATED 0
#define TIPK_CONF_BOUND     1
int     tipk_spd_factor(const float* hess, const float* row_scale, int64_t n_rows, int dim, float* out_l, float* out_w,
                        int32_t* status, tipk_stream_t stream);
int     tipk_distmult_pair_conf_topk_supported(int64_t n_nodes, int dim, int64_t n_rel, int k);
int     tipk_distmult_pair_conf_topk(const float* z, int64_t n_nodes, int dim, const float* rel_w, const float* w_fac,
                                     int64_t n_rel, const int32_t* pair_u, const int32_t* pair_v /* device */, int64_t n_pairs,
                                     const int64_t* known_pair_keys, const int64_t* known_pair_ptr, const int32_t* known_rel,
                                     int64_t n_known_pairs /* nullable together */, int k, int mode, float c,
                                     float* out_key, int32_t* out_rel, float* out_logit, float* out_var /* [n_pairs x k] */,
                                     float* dense_logit, float* dense_var /* [n_pairs x n_rel], nullable together */,
                                     tipk_stream_t stream);

/* 4q. Fit of the embedding of NEW drugs to their recorded interactions (serving; no reference call site): the dual of 4m.
 *     The embeddings z of the training graph's drugs and the DistMult decoder rows rel_w of 4a stay frozen; the unknown is
 *     the row x of a drug that is not a node of the graph, and a term is a CELL (partner v, side effect r).
 *
 *   Objective of new drug a with row x and prior centre c_a, s(v,r) = sum_k x[k] z[v,k] rel_w[r,k]:
 *     L_a(x) = sum_{distinct recorded cells p} wpos_p softplus(-s_p)
 *            + dense_w[a] * sum_{(v,r) in [0,n) x [0,R) NOT recorded} softplus(s)  +  l2/2 |x - c_a|^2
 *   evaluated as  dense_w[a] * sum over ALL n R cells of softplus(s)  -- a mask-free stream --  plus, per distinct recorded
 *   cell, wpos_p softplus(-s_p) - wneg_p softplus(s_p): wpos = multiplicity / P_a, wneg = dense_w[a] = neg_weight / N_a,
 *   N_a = n R - the distinct recorded cells (tip_amd.ops.drug_fit_csr builds them).  DistMult is symmetric: a cell has no
 *   direction.  The drug's pair with itself and pairs among new drugs are not part of the objective (the approximation of
 *   4k).  s is linear in x, so L_a is convex in dim unknowns; the feature of a cell is f = z[v] * rel_w[r].
 *
 *   tipk_distmult_drug_fit_stats.  Input, DEVICE: z [n_nodes x dim] and rel_w [n_rel x dim], dense, 16-byte aligned; the
 *   trial rows x [n_fit x dim]; dense_w fp32 [n_fit]; the distinct recorded cells as CSR: rec_ptr int64 [n_fit + 1], rec_v
 *   in [0, n_nodes) / rec_r in [0, n_rel) int32 [n_rec] (the caller's contract; an id outside is clamped, nothing is read
 *   out of bounds), rec_wpos / rec_wneg fp32 [n_rec]; prior [n_fit x dim], nullable (NULL: zeros); l2 >= 0; active int32
 *   [n_fit], nullable (NULL: every drug).  Output: loss [n_fit], grad [n_fit x dim], hess [n_fit x dim x dim] (row-major,
 *   both triangles), the l2 terms included.  Rows of an inactive drug are NOT touched.
 *   Arithmetic, fp32.  Feature f_k = z[v,k] * rel_w[r,k] rounded once; logit: acc = fmaf(f_k, x[k], acc), k ascending from
 *   +0.0f; softplus, sigma and sigma' from one expf exactly as in 4m.  Terms: loss c softplus, gradient c sigma f_i,
 *   Hessian c sigma' f_i f_j with c = dense_w[a].
 *   Summation order.  RECTANGULAR tiles of 64 partners x 64 side effects are numbered partner-block major; the tiles are
 *   cut into tipk_distmult_drug_fit_slabs(n_nodes, dim, n_rel, n_fit) SLABS of equal length (the last may be shorter).  In
 *   a tile wavefront q of 4 owns the partners v = 16 q .. 16 q + 15, in ascending order; within a partner the gradient and
 *   Hessian entries take the 64 side effects in r order on v_mfma_f32_16x16x4_f32 with the cells as K (an exact fmaf
 *   chain), the loss lane r adds its own term and the 64 lanes are summed at the end of the slab by the halving tree.  One
 *   accumulator per (slab, wavefront) runs through the slab: at most 1 024 terms per tile.  Then, per output, the 4 * slabs
 *   partials are added in ascending (slab, wavefront) order from +0.0f; the recorded cells are summed in chunks of 256 (a
 *   chain from +0.0f in list order, the chunk totals added in ascending order from +0.0f); result = dense + sparse, then
 *   + l2 term with d_k = x_k - c_k rounded once (loss: l2/2 times the fmaf chain of d_k^2; gradient: + l2 d_i; Hessian
 *   diagonal: + l2).
 *   tipk_distmult_drug_fit_max_chain(n_nodes, dim, n_rel, n_fit) = D, the largest number of fp32 additions a term passes
 *   through:  max(1 024 * tiles per slab + 6 + 4 * slabs,  256 + ceil(n R / 256)) + 2.
 *   Slabs and D depend on (n_nodes, dim, n_rel, n_fit) alone.  No floating-point atomics, no workgroup waits for another:
 *   the results are BITWISE repeatable call to call.
 *   Every drug streams every cell, whatever its dense_w.  A NaN logit makes every statistic of ITS drug NaN and touches no
 *   other drug: a NaN in z or rel_w reaches every drug, a NaN in one trial row only that drug.
 *   An INFINITE z[v,k] (no NaN logit: x[a,k] != 0, column k of rel_w without a zero, nothing else infinite) gives logits
 *   of +-inf on every cell of partner v: for every drug with dense_w[a] > 0, grad[k] and row k and column k of hess are
 *   non-finite (+inf or NaN: sigma' = 0 meets an infinite feature) and every other entry of grad and hess stays finite, so
 *   tipk_newton_step ends that drug with status 3; the loss is non-finite as soon as one unrecorded cell has the logit +inf
 *   or one recorded cell -inf.  Nothing finite is invented.  (A drug with dense_w[a] == 0 multiplies the infinite terms of
 *   the stream by zero: its statistics are NaN where those of the others are infinite.)
 *   Work: a dense launch of slabs x ceil(n_fit / 4) workgroups of 256 threads -- the feature of a cell is computed once
 *   for the 4 drugs of the block; the tile's z rows and rel_w rows are staged in LDS (rows 16-byte aligned, stride width +
 *   4 floats) -- then a finishing launch of one workgroup per drug.  A workgroup whose drugs are all inactive returns at
 *   once.  Nothing of size n R reaches memory.
 *   workspace: tipk_distmult_drug_fit_workspace_bytes(n_nodes, dim, n_rel, n_fit) bytes (-1: unsupported; n_fit == 0: 0),
 *   which also holds the state of tipk_distmult_drug_fit; the statistics entry uses its head.
 *
 *   tipk_distmult_drug_fit.  Enqueues one initialising launch (start = init [n_fit x dim]; NULL: the prior; both NULL:
 *   zeros) and max_iter + 1 (statistics, tipk_newton_step of 4m) pairs on `stream`; the active mask makes a finished drug's
 *   workgroups return at once.  Output: out_x [n_fit x dim], out_loss [n_fit], out_grad [n_fit x dim] = the accepted row
 *   and its statistics, out_info int32 [n_fit x 4] as in 4m (status 0 after max_iter + 1 evaluations: not converged);
 *   out_hess [n_fit x dim x dim], nullable: the Hessian of the ACCEPTED row -- one more statistics pair at out_x after the
 *   last step, so its bits are those of tipk_distmult_drug_fit_stats at out_x.
 *   Supported: 1 <= n_nodes, 1 <= n_rel, n_nodes * n_rel < 2^31, dim % 4 == 0 in 4..32 (widths below 16 | 32 zero-padded
 *   on chip), 1 <= n_fit <= 65 536; z and rel_w 16-byte aligned.
 *   Status: TIPK_EINVAL -- before anything is launched or written -- for a negative size, n_nodes, n_rel or dim < 1, l2 < 0
 *   or NaN, gtol < 0 or NaN, max_iter < 0, a NULL required pointer (with n_fit > 0: everything but `prior`, `active`,
 *   `init`, `out_hess` and, with n_rec == 0, the four cell arrays); then TIPK_EUNSUPPORTED outside the supported range;
 *   n_fit == 0 is TIPK_OK with no launch and nothing written.
 *   Nothing lives in host memory: the entries do NOT synchronise or allocate and may be captured into a hipGraph
 *   (sequential launches, no parallel branches).
 */
int     tipk_distmult_drug_fit_supported(int64_t n_nodes, int dim, int64_t n_rel, int64_t n_fit);
int64_t tipk_distmult_drug_fit_slabs(int64_t n_nodes, int dim, int64_t n_rel, int64_t n_fit);            /* -1 unsupported */
int64_t tipk_distmult_drug_fit_max_chain(int64_t n_nodes, int dim, int64_t n_rel, int64_t n_fit);        /* -1 unsupported */
int64_t tipk_distmult_drug_fit_workspace_bytes(int64_t n_nodes, int dim, int64_t n_rel, int64_t n_fit);  /* -1 unsupported */
int     tipk_distmult_drug_fit_stats(const float* z, int64_t n_nodes, int dim, const float* rel_w, int64_t n_rel,
                                     const float* x, int64_t n_fit, const float* dense_w,
                                     const int64_t* rec_ptr /* [n_fit+1] */, const int32_t* rec_v, const int32_t* rec_r,
                                     const float* rec_wpos, const float* rec_wneg, int64_t n_rec,
                                     const float* prior /* nullable: zeros */, float l2, const int32_t* active /* nullable */,
                                     float* loss, float* grad, float* hess, void* workspace, tipk_stream_t stream);
int     tipk_distmult_drug_fit(const float* z, int64_t n_nodes, int dim, const float* rel_w, int64_t n_rel, int64_t n_fit,
                               const float* dense_w, const int64_t* rec_ptr /* [n_fit+1] */, const int32_t* rec_v,
                               const int32_t* rec_r, const float* rec_wpos, const float* rec_wneg, int64_t n_rec,
                               const float* prior /* nullable: zeros */, float l2,
                               const float* init /* nullable: the prior */, int max_iter, float gtol,
                               float* out_x, float* out_loss, float* out_grad, int32_t* out_info,
                               float* out_hess /* nullable */, void* workspace, tipk_stream_t stream);

/* 4r. Calibration of the DistMult probabilities: a Platt map per side effect (serving; no reference call site).  The model
 *     is trained on one uniform negative per positive, so sigma(logit) sits at a 1:1 class balance; the map
 *     logit' = a_r logit + b_r is fitted on held-out positives against ALL unrecorded pairs at their true prevalence.  It
 *     keeps every ranking inside a side effect (a_r > 0) and moves the level.
 *
 *   A QUERY q names a relation q_rel[q].  Its CELLS are the unordered pairs u < v of [0, n); three sets partition them:
 *     TRAIN  the cells recorded for the relation in training, in either direction;
 *     POS    the distinct given calibration pairs with u != v that are not in TRAIN;
 *     NEG    every other cell.                                       M = |POS| + |NEG|.
 *   Logit s(u,v), u < v, with exactly the arithmetic of wg_score_tile (4c, 4h): x = z[u,k] * w[k] rounded once, acc =
 *   fmaf(x, z[v,k], acc), k ascending from +0.0f -- the screen's logit, bit for bit.  With t = fmaf(a, s, b):
 *     L_q(a, b) = 1/M [ sum_POS softplus(-t) + sum_NEG softplus(t) ] + l2/2 (a - 1)^2
 *   softplus exact (no epsilon), the intercept not penalised; l2 only bounds a on a separable list.  Convex in (a, b).
 *   Evaluated as  dense_w[q] * sum over ALL cells of softplus(t)  -- a mask-free stream --  plus, per LISTED cell (the merged,
 *   sorted list of the distinct TRAIN and POS cells, u < v: the caller's contract), wpos_p softplus(-t_p) + wneg_p
 *   softplus(t_p):  dense_w = 1/M; a TRAIN cell has wpos = 0, wneg = -1/M; a POS cell wpos = 1/M, wneg = -1/M
 *   (tip_amd.ops.calibration_lists builds them; M == 0: all three 0).  The logit of a listed cell is recomputed with the
 *   same chain, so what the stream added is taken out at the same bits of s.
 *
 *   tipk_distmult_calibrate_stats.  Input, DEVICE: z [n_nodes x dim] dense, 16-byte aligned; rel_w [n_rel x dim]; q_rel
 *   int32 [n_q] in [0, n_rel); the trial maps ab [n_q x 2] = (a, b); dense_w fp32 [n_q]; the listed cells as CSR: pair_ptr
 *   int64 [n_q + 1], pair_u / pair_v int32 [n_pairs] in [0, n_nodes) (an id outside, also of q_rel, is clamped: nothing is
 *   read out of bounds), pair_wpos / pair_wneg fp32 [n_pairs]; l2 >= 0; active int32 [n_q], nullable (NULL: every query).
 *   Output: loss [n_q], grad [n_q x 2] = (dL/da, dL/db), hess [n_q x 2 x 2] (row-major, both triangles), the l2 terms
 *   included: the layout tipk_newton_step(dim = 2, ...) reads.  Rows of an inactive query are NOT touched.
 *   Arithmetic.  Per cell, fp32, from one expf as in 4m: e = expf(-|t|), r = 1.0f / (1.0f + e), softplus(t) = fmaxf(t, 0) +
 *   log1pf(e), sigma = r (t >= 0) | e r, sigma' = e r r; the six terms softplus, sigma s, sigma, (sigma' s) s, sigma' s,
 *   sigma', each product rounded once.
 *   Summation order.  The tiles of 64 x 64 cells (u-block, v-block >= u-block; u-block major) are dealt to
 *   tipk_distmult_calibrate_splits(n_nodes, dim, n_q) PARTS per query: part x of S owns the tiles [T x / S, T (x + 1) / S).
 *   In a tile thread (ty, tx) of 16 x 16 owns the cells (4 ty + i, 4 tx + j) and adds their terms in fp32 in (i, j) order,
 *   i major, from +0.0f; a cell with u >= v or v >= n adds +0.0f.  The tile's sum goes onto an fp64 accumulator of the
 *   thread that runs through the part; at its end the 64 lanes of a wavefront are added by the halving tree (lane l +=
 *   lane l + 32, 16, .., 1), the 4 wavefronts in ascending order from 0.0.  The finishing launch adds the parts in ascending
 *   order from 0.0 (fp64); a listed cell's terms are scaled by wpos | wneg in fp64, thread x of 256 adds the cells x, x +
 *   256, ... of the list in that order, threads and wavefronts are added as above;  result = dense_w * dense + sparse
 *   + the l2 term (loss: l2/2 (a - 1)^2; grad[0]: l2 (a - 1); hess[0][0]: l2), all in fp64, rounded to fp32 ONCE.
 *   tipk_distmult_calibrate_max_chain(n_nodes, dim, n_q) = D = 18, the most fp32 additions a term passes through: the 16
 *   cells of a thread in a tile and the final rounding, + 1 for all the fp64 additions together.
 *   Parts and D depend on (n_nodes, dim, n_q) alone.  No floating-point atomics, no workgroup waits for another, no trip
 *   count depends on data: the results are BITWISE repeatable call to call.
 *   A weight of exactly 0 (dense_w, wpos, wneg, wpos + wneg for the Hessian) makes its term ABSENT: it adds 0 whatever the
 *   term is.  So a query with M == 0 has the l2 term alone, whatever its logits are.
 *   A NaN logit makes every statistic of ITS query NaN (M > 0) and touches no other query (a NaN row of z reaches every
 *   query with n >= 2, a NaN in a row of rel_w or in one (a, b) only the queries of that relation or that map).
 *   An INFINITE z[u,k] (no NaN logit; w[k] != 0, the other entries of column k != 0, a != 0) gives t = +-inf on the cells of
 *   row u: for a query with M > 0, grad[0], hess[0][0], hess[0][1] and hess[1][0] are non-finite (+-inf or NaN: sigma' = 0
 *   meets an infinite s), so tipk_newton_step ends that query with status 3; grad[1] and hess[1][1] stay finite; the loss is
 *   non-finite as soon as one cell has t = +inf or one POS cell t = -inf (a listed cell streamed at +inf is taken out
 *   again: NaN).  Nothing finite is invented.
 *   Work: a dense launch of n_q x parts workgroups of 256 threads -- the logits on the vector unit (the fp32 matrix cores
 *   offer the same rate and do not overlap with it; the per-cell transform is the cost) --, then a finishing launch of one
 *   workgroup per query.  A workgroup of an inactive query returns at once.  Nothing of size n^2 reaches memory.
 *   workspace: tipk_distmult_calibrate_workspace_bytes(n_nodes, dim, n_q) bytes, 8-byte aligned (-1: unsupported; n_q ==
 *   0: 0), which also holds the state of tipk_distmult_calibrate; the statistics entry uses its head.
 *
 *   tipk_distmult_calibrate.  Enqueues one initialising launch (start = init [n_q x 2]; NULL: the identity (1, 0)) and
 *   max_iter + 1 (statistics, tipk_newton_step of 4m with dim = 2, through its C entry, as it is) pairs on `stream`; the
 *   active mask makes a finished query's workgroups return at once.  Output: out_ab [n_q x 2], out_loss [n_q], out_grad
 *   [n_q x 2] = the accepted map and its statistics, out_info int32 [n_q x 4] as in 4m (status 0 after max_iter + 1
 *   evaluations: not converged).
 *   Supported: 1 <= n_nodes <= 46 340, dim % 4 == 0 in 4..256, 1 <= n_q <= 65 536, n_rel < 2^31; z 16-byte aligned.
 *   Status: TIPK_EINVAL -- before anything is launched or written -- for a negative size, n_nodes, dim or n_rel < 1, l2 < 0
 *   or NaN, gtol < 0 or NaN, max_iter < 0, a NULL required pointer (with n_q > 0: everything but `active`, `init` and, with
 *   n_pairs == 0, the four cell arrays); then TIPK_EUNSUPPORTED outside the supported range; n_q == 0 is TIPK_OK with no
 *   launch and nothing written.
 *   Nothing lives in host memory: the entries do NOT synchronise or allocate and may be captured into a hipGraph
 *   (sequential launches, no parallel branches).
 *   Applying the map needs no kernel: with z' = [z | 1 0 0 0] and w'_r = [a_r w_r | b_r 0 0 0] every DistMult entry of
 *   section 4 computes a_r s + b_r up to rounding -- the constant column is the last term of the ascending fma chain.
 */
int     tipk_distmult_calibrate_supported(int64_t n_nodes, int dim, int64_t n_q);
int64_t tipk_distmult_calibrate_splits(int64_t n_nodes, int dim, int64_t n_q);           /* -1 unsupported */
int64_t tipk_distmult_calibrate_max_chain(int64_t n_nodes, int dim, int64_t n_q);        /* -1 unsupported */
int64_t tipk_distmult_calibrate_workspace_bytes(int64_t n_nodes, int dim, int64_t n_q);  /* -1 unsupported */
int     tipk_distmult_calibrate_stats(const float* z, int64_t n_nodes, int dim, const float* rel_w, int64_t n_rel,
                                      const int32_t* q_rel, const float* ab /* [n_q x 2] */, int64_t n_q,
                                      const float* dense_w, const int64_t* pair_ptr /* [n_q+1] */, const int32_t* pair_u,
                                      const int32_t* pair_v, const float* pair_wpos, const float* pair_wneg, int64_t n_pairs,
                                      float l2, const int32_t* active /* nullable */, float* loss, float* grad, float* hess,
                                      void* workspace, tipk_stream_t stream);
int     tipk_distmult_calibrate(const float* z, int64_t n_nodes, int dim, const float* rel_w, int64_t n_rel,
                                const int32_t* q_rel, int64_t n_q, const float* dense_w,
                                const int64_t* pair_ptr /* [n_q+1] */, const int32_t* pair_u, const int32_t* pair_v,
                                const float* pair_wpos, const float* pair_wneg, int64_t n_pairs, float l2,
                                const float* init /* nullable: (1, 0) */, int max_iter, float gtol,
                                float* out_ab, float* out_loss, float* out_grad, int32_t* out_info, void* workspace,
                                tipk_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * 5. Typed negative sampling on device -- replaces typed_negative_sampling / negative_sampling,
 *    src/neg_sampling.py:5-26 (K11: host numpy + one D2H copy per relation).
 *
 * For every positive position e of relation r (rel_ptr[r] <= e < rel_ptr[r+1]) draw a pair
 * uniformly from n_nodes^2 (with replacement, self pairs allowed, as np.random.choice does) and
 * redraw while it equals a positive pair OF THE SAME RELATION.  Randomness: Philox4x32-10, key = (seed_lo, seed_hi);
 * n^2 < 2^32: ONE call (counter = (e >> 2, attempt, 0)) serves the four positions 4q .. 4q + 3, a candidate is the high
 * word of x * n^2 and is redrawn when the low word is below (2^32 - n^2) mod n^2 (exactly uniform); larger node sets:
 * counter = (e, attempt, 0), candidate = mulhi64(r0 | r1<<32, n^2) -- specified bit-exactly in
 * oracle/philox_sampler.py.  `pos_key_sorted` holds u*n+v of each relation's positives sorted ascending within the
 * relation (int64); `pos_key32` (nullable) the same keys as uint32, in any order inside a relation: what the bitmap
 * route reads when given (half the bytes).  After 64 rejected attempts the 64th candidate is kept (probability <
 * density^64).
 * wg_unit_ptr [n_wg + 1] / wg_units [n_units][3] (nullable, int32): edge-balanced deal of UNITS = (relation, first
 * position, end position) to n_wg workgroups -- the units tile [0, n_positions), a unit lies inside one relation (a
 * relation larger than a workgroup's share is cut into several units); with it and n_nodes^2 bits <= 150 KB each
 * workgroup tests candidates against an LDS bitmap of its relation's positives instead of searching the sorted keys
 * (same output bit for bit, ~6x faster on BioSNAP).
 * call_counter != NULL: a sampler STREAM whose state lives on the device, uint64[2] = { position, seed }:
 * the Philox key is splitmix64(state[1] + (state[0] + 1) * 0x9E3779B97F4A7C15) and the host `seed`
 * argument is ignored -- a captured hipGraph draws new negatives on every replay
 * and re-seeding after capture (a device-side write of the words) takes effect in the replays.  The position moves
 * on either by `tipk_counter_advance` on state[0] (a launch of its own), or -- advance != 0, state then is uint64[3] =
 * { position, seed, ticket (0) } -- inside the sampling launch: its last workgroup to finish stores position + 1.
 * pos_offset (nullable, int64 [n_rel]): the Philox counter of position e of relation r is e + pos_offset[r] -- a rank
 * of a relation-sharded run passes (start of r's block in the WHOLE triple list) - rel_ptr[r], so that its negatives
 * are exactly the negatives the unsharded run draws for those relations, whatever the number of ranks.
 */
/* workgroups per CU the bitmap sampler is launched with for this node count (plan the units for CUs x this many workgroups):
 * 2 when two bitmaps of n_nodes^2 bits fit the LDS of a CU (512-thread workgroups), 1 (1024 threads), 0 = no bitmap route */
int tipk_negsample_wgs_per_cu(int64_t n_nodes);
int tipk_typed_negative_sampling(const int64_t* pos_key_sorted, const int64_t* rel_ptr /* [n_rel+1] */,
                                 int64_t n_rel, int64_t n_nodes, uint64_t seed,
                                 uint64_t* call_counter /* nullable device uint64[2 or 3], see above */, int advance,
                                 const int32_t* wg_unit_ptr /* nullable */, const int32_t* wg_units, int64_t n_wg,
                                 const int64_t* pos_offset /* nullable */, const uint32_t* pos_key32 /* nullable */,
                                 void* out_u, void* out_v, int idx_bytes,
                                 int64_t n_positions /* = rel_ptr[n_rel], host copy */,
                                 tipk_stream_t stream);

int tipk_counter_advance(uint64_t* call_counter /* device */, tipk_stream_t stream);   /* *counter += 1 */

/* --------------------------------------------------------------------------------------------
 * 6. Per-relation ranking metrics on device -- replaces the loop of
 *    TIP.compute_auprc_auroc_ap_by_et (src/layers.py:355-375) over sklearn's roc_auc_score,
 *    average_precision_score and auc(precision_recall_curve) (src/utils.py:86-93): 1 097 D2H copies
 *    and sorts on the host.
 *
 * Relation r scores pos_score[range_ptr[r] : range_ptr[r+1]] against the same slice of neg_score
 * (labels 1 / 0).  out is fp64 [3][n_rel] = (AUPRC, AUROC, AP) rows.  Ties share one operating
 * point, exactly as sklearn's curves do.  max_pairs (host) = largest slice; 2*max_pairs <= 16384
 * (one workgroup sorts a relation in LDS), else TIPK_EUNSUPPORTED and the caller evaluates on the host.
 *
 * Score policy (tip_amd/utils.py follows the same one on the host path):
 *   zeros     -0.0 and +0.0 are one score, hence one threshold (as sklearn and numpy compare them);
 *   +-inf     ordinary scores, the largest and the smallest; equal infinities tie;
 *   NaN       a relation whose block holds a NaN score reports NaN in all three metrics (sklearn raises; a
 *             diverged model must not report an AUROC).  The other relations of the launch are unaffected;
 *   empty     a relation with range_ptr[r+1] <= range_ptr[r] reports NaN in all three metrics;
 *   max_pairs sizes the LDS of the launch.  A relation larger than an understated max_pairs is not sorted and
 *             reports NaN (the kernel decides that from range_ptr alone and never indexes LDS beyond its size).
 * Every cell of out is written by every successful launch.
 */
int tipk_rank_metrics(const float* pos_score, const float* neg_score, const int64_t* range_ptr /* [n_rel+1] */,
                      int64_t n_rel, int64_t max_pairs, double* out, tipk_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * 7. Train / test split on device -- replaces `process_edges`, src/utils.py:35-65 (host numpy: one
 *    `np.random.binomial(1, p, E_r)` per relation from the global Mersenne state, Python lists, then
 *    `to_bidirection`), SURVEY.md section 8(f) item 2.
 *
 *    The undirected pairs of all relations arrive concatenated (pairs_u/pairs_v [n_pairs], 2-byte or
 *    8-byte ids; rel_ptr [n_rel + 1]).  Pair i is a TRAINING pair iff
 *        Philox4x32-10(counter = (i lo, i hi, 0, 0x53504C54), key = (seed lo, seed hi)).x0 < floor(p * 2^32)
 *    (p = 1 keeps every pair) -- specified bit-exactly in oracle/philox_split.py.
 *    tipk_split_flags  writes take[i] (1 = train) and ADDS the kept pairs per relation to n_train[r]
 *                      (uint64, caller zeroes).
 *    tipk_split_scatter  with train_ptr / test_ptr [n_rel + 1] = offsets of every relation's block of
 *                      DIRECTED edges in the outputs (2 * kept, 2 * dropped: exclusive sums the caller
 *                      forms from n_train), writes per relation r the kept pairs in list order as
 *                      [ (u,v) ... | (v,u) ... ] into train_u/v with train_et = r, the dropped ones the same
 *                      way into test_* -- the layout of `to_bidirection` (src/utils.py:17-23, :53).
 *    Outputs are int64 (the reference's dtype). */
int tipk_split_flags(const int64_t* rel_ptr, int64_t n_rel, int64_t n_pairs, double p_train, uint64_t seed,
                     uint8_t* take, uint64_t* n_train, tipk_stream_t stream);
int tipk_split_scatter(const void* pairs_u, const void* pairs_v, int idx_bytes, const int64_t* rel_ptr, int64_t n_rel,
                       const uint8_t* take, const int64_t* train_ptr, const int64_t* test_ptr,
                       int64_t* train_u, int64_t* train_v, int64_t* train_et,
                       int64_t* test_u, int64_t* test_v, int64_t* test_et, tipk_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * 8. One-shot all-reduce over peer-mapped mailboxes -- the xGMI-aware exchange of the relation-sharded step
 *    (north_star: "the D-D pass shards by relation-id across the 8 GPUs of one node with an ... all-reduce of drug
 *    embeddings over xGMI"; the reference is single-GPU, README.md:58).  SUM of one fp32 buffer of n <= max_floats
 *    elements over `world` ranks (one process per GPU), result identical bit for bit on every rank (slots added in
 *    rank order).  tip_amd/csrc/tipk_peer.hip describes the protocol.
 *      tipk_peer_mailbox_bytes   size of one rank's mailbox (two halves of world slots + flags, + the call counter);
 *      tipk_peer_alloc / _free   the mailbox: UNCACHED device memory, zeroed (explicit allocation entry points: the
 *                                only ones of the library -- such memory cannot come from the caller's allocator);
 *      tipk_ipc_get_handle / _open / _close   hipIpc handle (64 bytes) of the own mailbox / mapping of a peer's;
 *      tipk_peer_allreduce       data [n] <- sum over ranks; mailboxes = HOST array [world] of the mailboxes' addresses
 *                                in THIS process (own one at [rank]); every rank must call with the same n, in the same
 *                                order.  Two launches (exchange + call counter), no host synchronisation: capturable.
 */
int64_t tipk_peer_mailbox_bytes(int world, int64_t max_floats);
int tipk_peer_alloc(int64_t bytes, void** ptr);
int tipk_peer_free(void* ptr);
int tipk_ipc_get_handle(void* ptr, void* handle_out /* 64 bytes, host */);
int tipk_ipc_open(const void* handle /* 64 bytes, host */, void** ptr);
int tipk_ipc_close(void* ptr);
int tipk_peer_allreduce(float* data, int64_t n, void* const* mailboxes /* host [world] */, int rank, int world,
                        int64_t max_floats, tipk_stream_t stream);
/*      BOUNDED WAIT: the flag wait of an exchange has a wall-clock budget (default 2 000 ms).  A rank whose peer died,
 *      skipped a call or took another collective does not spin for ever: the kernel records {sequence number << 32 |
 *      (missing rank + 1) << 16 | chunk} in the ERROR WORD of its own mailbox (first record wins) and finishes with
 *      whatever the slots hold.  tipk_peer_status copies that word to the host (0 = every wait was served; a synchronous
 *      8-byte copy: call it where the host synchronises anyway, never inside a capture); the caller must treat a
 *      non-zero word as fatal for the process group.  tipk_peer_set_timeout_ms: the budget of later launches (1 ... 600 000),
 *      ONE value for every exchange of the process (a short budget for a self-test, then a production budget that outlasts
 *      the host-side skew between ranks: tip_amd/dist.py leaves 60 000 ms behind). */
int tipk_peer_set_timeout_ms(int64_t ms);
int tipk_peer_status(void* mailbox, int world, int64_t max_floats, uint64_t* error_word /* host */);

/* --------------------------------------------------------------------------------------------
 * 9. Optimizer step of the training loop -- replaces `optimizer.step()` of tip.py:24-30
 *    (torch.optim.Adam(model.parameters(), lr=0.01): amsgrad off, maximize off, L2 weight decay).
 *    ONE launch over a list of fp32 tensors (host arrays [n_tensors] of device pointers; element i of params, grads,
 *    exp_avg, exp_avg_sq must share one dense layout of numel[i] elements):
 *        g += weight_decay * p;  m += (1 - beta1) (g - m);  v = beta2 v + (1 - beta2) g g;
 *        p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps),      t = *steps[i] + 1
 *    in fp32, every hyper-parameter constant -- beta2, 1 - beta1, 1 - beta2, weight_decay, eps, lr / (1 - beta1^t),
 *    1 / sqrt(1 - beta2^t) -- formed in double and rounded ONCE to fp32 (never 1.0f - (float)beta: that is 216 u = 1.3e-5
 *    off for beta2 = 0.999); `/` and sqrt correctly rounded.  tests/adam_spec.py holds the step to the rounding bound of that.
 *    steps: host array [n_tensors] of device uint64 words, the steps tensor i has made (torch keeps the count per
 *    parameter: one without a gradient sits the step out); ticket: device uint64[528], zeros (left zeroed; 33 ticket words, one per 128-byte line).  The launch's last workgroup adds 1 to
 *    the counts of its tensors -- a captured hipGraph keeps counting on replay.  Tensors with numel 0 are skipped (their
 *    count does not move).  The addresses are kernel arguments (48 tensors per launch, longer lists take several
 *    launches): nothing is uploaded, nothing allocated. */
int tipk_adam_step(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                   float* const* exp_avg_sq, const int64_t* numel, uint64_t* const* steps, uint64_t* ticket /* device */,
                   double lr, double beta1, double beta2, double eps, double weight_decay, tipk_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * 10. Op-level entries (round 6): a graph handle that OWNS the preprocessed buffers of a D-D graph
 *     and ONE call per pass of an R-GCN layer -- reference MyRGCNConv2.forward(x, edge_index, edge_type, range_list)
 *     (src/layers.py:157-188; with edge_type instead of range_list: MyRGCNConv.forward, :76-99) and its autograd -- for a host
 *     that is not this package's Python: raw device pointers + handle + caller-supplied workspace + stream.
 *
 *     tipk_graph_build (the only entry of the library that allocates, and that synchronises: preprocessing, once per graph):
 *         edge_index [2][n_edges] (row 0 sources, row 1 destinations), and either range_list [n_rel][2] (start, end) of
 *         consecutive blocks, as MyRGCNConv2 takes it, or edge_type [n_edges]; idx_bytes 4 | 8 for all three; the arrays may
 *         live on the device or on the host.  in_degree (nullable, float [n_nodes]): the in-degree of the WHOLE graph when the
 *         edge list is one rank's shard of the relations.  Ids out of range -> TIPK_EINVAL (the reference raises IndexError).
 *         The handle holds two CSRs (rows of the output by destination; rows (relation, source) by destination list) and
 *         1 / max(1, in-degree): edge order inside a row = order of the edge list, so every pass is bitwise reproducible.
 *     tipk_rgcn_fwd:   out = relu?( D^-1 sum_r A_r X W_r + X root ),  W_r = sum_b att[r, b] basis[b]
 *         x [N x d_in] (row stride ld_x), basis [n_bases x d_in x d_out], att [R x n_bases], root [d_in x d_out] contiguous.
 *     tipk_rgcn_bwd:   from grad_out [N x d_out]; out_relu (nullable) = the forward output when relu was set (its mask is
 *         applied first) -> g_x [N x d_in], g_basis, g_att, g_root (shapes of the parameters, contiguous, overwritten).
 *     workspace: tipk_rgcn_workspace_bytes(graph, d_in, d_out, n_bases) bytes, 16-byte aligned, caller-owned, reusable
 *         between calls on one stream (the backward pass recomputes XB: nothing is kept across the two calls but the
 *         caller's own X, parameters and -- with relu -- the output).
 *     Routes.  Generic (any shapes): basis-first, transform-then-gather, Y = att . XB [R N x d_out] the largest temporary.
 *     PAIR FORM (what the PyTorch modules take at BioSNAP size; both D-D layers forward + backward through these entries:
 *     1.9 ms on the generic route, 0.18 ms in pair form -- tools/bench_c_abi.py, `op_level_c_abi` on the bench line):
 *     tipk_graph_prepare_rgcn(graph, n_bases, d_out) builds the plans of the LDS-resident pair form for that layer shape --
 *     on the host, with the C++ builders of section 10c; allocates and synchronises like tipk_graph_build -- when the graph
 *     qualifies (<= 1 024 nodes, an att table [R x n_bases] that fits in LDS, n_bases and d_out the pair kernels support);
 *     TIPK_EUNSUPPORTED otherwise, and the generic route stays.  Call it once per layer shape BEFORE asking for the
 *     workspace size; tipk_rgcn_fwd / _bwd then run sections 1d + 2c (+ 2e) on the handle's plans.  tipk_graph_rgcn_route:
 *     0 generic, 1 pair-form forward (backward generic), 2 pair form both ways.  The handle keeps the edge list on the host
 *     (12 bytes per edge) for later prepare calls until tipk_graph_release_host.
 *     tipk_rgcn_bwd_ex(..., flags, stream): TIPK_RGCN_WORKSPACE_FROM_FWD = the workspace still holds what tipk_rgcn_fwd of THIS
 *     layer left in it (pair cells and XB: the caller ran nothing else on that workspace in between) -- the backward pass then
 *     skips recomputing them; tipk_rgcn_bwd = flags 0 (always safe).  On a prepared route the handle's gradient table is
 *     scratch of the backward call: one backward pass per handle at a time (calls on one stream are ordered anyway).
 *     The rule of every entry in this section: TIPK_OK implies correct numbers, for every stride the call accepts; otherwise a
 *     non-OK status (shape and argument checks fail before anything is written).  tipk_rgcn_fwd takes the same route for every ld_out (a padded `out` of the pair
 *     form is written densely into the workspace and copied with its stride), so a FROM_FWD backward pass always finds the
 *     cells and XB of its own route.
 */
#define TIPK_RGCN_WORKSPACE_FROM_FWD 1
typedef struct tipk_graph tipk_graph;
int tipk_graph_build(const void* edge_index, const void* edge_type /* nullable */, const void* range_list /* nullable */,
                     int idx_bytes, int64_t n_edges, int64_t n_nodes, int64_t n_rel, const float* in_degree /* nullable */,
                     tipk_graph** graph_out);
int tipk_graph_destroy(tipk_graph* graph);
int tipk_graph_info(const tipk_graph* graph, int64_t* n_nodes, int64_t* n_rel, int64_t* n_edges,
                    const float** inv_degree /* device, owned by the handle */);
int64_t tipk_rgcn_workspace_bytes(const tipk_graph* graph, int d_in, int d_out, int n_bases);
int tipk_rgcn_fwd(const tipk_graph* graph, const float* x, int64_t ld_x, int d_in, const float* basis, const float* att,
                  const float* root, int n_bases, int d_out, int relu, float* out, int64_t ld_out,
                  void* workspace, int64_t workspace_bytes, tipk_stream_t stream);
int tipk_rgcn_bwd(const tipk_graph* graph, const float* x, int64_t ld_x, int d_in, const float* basis, const float* att,
                  const float* root, int n_bases, int d_out, const float* grad_out, int64_t ld_g,
                  const float* out_relu /* nullable */, int64_t ld_relu, float* g_x, int64_t ld_gx, float* g_basis, float* g_att,
                  float* g_root, void* workspace, int64_t workspace_bytes, tipk_stream_t stream);
int tipk_rgcn_bwd_ex(const tipk_graph* graph, const float* x, int64_t ld_x, int d_in, const float* basis, const float* att,
                     const float* root, int n_bases, int d_out, const float* grad_out, int64_t ld_g,
                     const float* out_relu /* nullable */, int64_t ld_relu, float* g_x, int64_t ld_gx, float* g_basis, float* g_att,
                     float* g_root, void* workspace, int64_t workspace_bytes, int flags, tipk_stream_t stream);
int tipk_graph_prepare_rgcn(tipk_graph* graph, int n_bases, int d_out);
int tipk_graph_rgcn_route(const tipk_graph* graph, int n_bases, int d_out);
int tipk_graph_release_host(tipk_graph* graph);

/* 10b. The other two layer kinds of the path behind the same kind of handle (tipk_graph_destroy frees them all):
 *   GCNConv as PPEncoder uses it (PyG 2.0.1 semantics, src/layers.py:386-394): tipk_gcn_graph_build forms
 *   A_hat = D^-1/2 (A + I) D^-1/2 -- existing self loops replaced by exactly one unit loop per node, D = in-degree incl. the
 *   loop, flow source -> target -- as two weighted CSRs.
 *     tipk_gcn_fwd:  out = relu?( A_hat (x W^T) + bias );  x = NULL: identity features (lin(I) = W^T, read in place: w_so must be 1);
 *                    weight element (o, i) at weight[o * w_so + i * w_si] (any layout of the [out, in] parameter).
 *     tipk_gcn_bwd:  grad_out (masked with out_relu > 0 when given) -> g_x (nullable; needs x), g_weight (element (o, i) at
 *                    g_weight[o * gw_so + i * gw_si]; dense x: gw_si must be 1; identity: gw_so must be 1 -- d W is the transposed
 *                    aggregate written in place), g_bias (nullable).
 *   MyHierarchyConv (src/layers.py:196-247): tipk_hier_graph_build keeps the edges that end in rows [n_source, n_all) of the
 *   concatenated node space; tipk_hier_fwd: out [n_all - n_source x d_out] = mean over incoming edges of x [n_all x d_in] . weight
 *   [d_in x d_out]; tipk_hier_bwd -> g_x [n_all x d_in] (nullable), g_weight.
 *   Workspaces: tipk_gcn_workspace_bytes / tipk_hier_workspace_bytes, 16-byte aligned, caller-owned.  (The fused objective of the
 *   DistMult decoder is one C call already: tipk_distmult_loss_store, section 4.) */
int tipk_gcn_graph_build(const void* edge_index, int idx_bytes, int64_t n_edges, int64_t n_nodes, tipk_graph** graph_out);
int64_t tipk_gcn_workspace_bytes(const tipk_graph* graph, int d_in, int d_out);
int tipk_gcn_fwd(const tipk_graph* graph, const float* x /* nullable */, int64_t ld_x, int d_in, const float* weight, int64_t w_so,
                 int64_t w_si, const float* bias /* nullable */, int d_out, int relu, float* out, int64_t ld_out,
                 void* workspace, int64_t workspace_bytes, tipk_stream_t stream);
int tipk_gcn_bwd(const tipk_graph* graph, const float* x /* nullable */, int64_t ld_x, int d_in, const float* weight, int64_t w_so,
                 int64_t w_si, int d_out, const float* grad_out, int64_t ld_g, const float* out_relu /* nullable */, int64_t ld_relu,
                 float* g_x /* nullable */, int64_t ld_gx, float* g_weight, int64_t gw_so, int64_t gw_si, float* g_bias /* nullable */,
                 void* workspace, int64_t workspace_bytes, tipk_stream_t stream);
int tipk_hier_graph_build(const void* edge_index, int idx_bytes, int64_t n_edges, int64_t n_all, int64_t n_source,
                          tipk_graph** graph_out);
int64_t tipk_hier_workspace_bytes(const tipk_graph* graph, int d_in, int d_out);
int tipk_hier_fwd(const tipk_graph* graph, const float* x, int64_t ld_x, int d_in, const float* weight, int d_out, float* out,
                  int64_t ld_out, void* workspace, int64_t workspace_bytes, tipk_stream_t stream);
int tipk_hier_bwd(const tipk_graph* graph, const float* x, int64_t ld_x, int d_in, const float* weight, int d_out,
                  const float* grad_out, int64_t ld_g, float* g_x /* nullable */, int64_t ld_gx, float* g_weight,
                  void* workspace, int64_t workspace_bytes, tipk_stream_t stream);

/* 10c. Plan construction in C++ (tip_amd/csrc/tipk_pairplan.hip), exposed as HOST arrays: the work lists of the wave-stream
 *     gathers (section 1d) and of the pair-form backward pass (section 2e) from index arrays in host memory -- the same arrays,
 *     bit for bit, as tip_amd/plan.py `build_stream_plan_rows` / `build_pair_bwd_plan` and tip_amd/layers.py `pair_link_words`
 *     (tests/test_host_plans.py).  The graph handle of section 10 builds its pair-form plans with these (tipk_graph_prepare_rgcn);
 *     a host that manages its own device buffers can upload them and call the kernel-level entries itself.
 *     Arrays by name -- stream plan: "wave_ptr", "cells", "ids" (uint16), "zero_ptr", "zero_rows"; pair backward plan: "slots",
 *     "node_desc", "tile_node", "part_first", "wg_part" and the gather's under "gather.<name>"; link words: "links".
 *     Scalars by name: "n_rows", "n_table", "n_bands", "n_edges", "n_wg", "lanes", "piece", "idx_unit", "row_bytes" (prefixed with
 *     "gather." on a pair plan) and "n_slots", "n_parts", "part_len", "n_alloc", "symmetric"; -1 = unknown name.
 *     wide_steps / row_bytes 0 = the defaults (16; lanes * 16). */
typedef struct tipk_host_plan tipk_host_plan;
int tipk_plan_stream_rows(const int64_t* out_row, const int64_t* tab_row, int64_t n_edges, int64_t n_rows, int64_t n_table,
                          int n_wg, int lanes, int piece, int wide_steps, int row_bytes, tipk_host_plan** plan_out);
int tipk_plan_pair_bwd(const int64_t* src, const int64_t* dst, const int64_t* rel, int64_t n_edges, int64_t n_nodes, int64_t n_rel,
                       const float* scale /* [n_nodes] 1 / in-degree */, int symmetric, int n_wg, int lanes, int piece,
                       tipk_host_plan** plan_out);
/* grouped gather plan of section 1 (plan.py `build_gather_plan` with group_slots = G > 0; chunk 0 = from the edge count):
 * arrays "row_id", "edge_w" (float; empty without weights), "items", "perm" (int64); scalars "n_items", "chunk", "group_slots". */
int tipk_plan_gather(const int64_t* out_row, const int64_t* table_row, const float* edge_w /* nullable */, int64_t n_edges,
                     int64_t n_out, int64_t n_table, int chunk, int group_slots, tipk_host_plan** plan_out);
int tipk_plan_link_words(const int64_t* src, const int64_t* dst, int64_t n_edges, int64_t n_nodes, tipk_host_plan** plan_out);
int tipk_host_plan_array(const tipk_host_plan* plan, const char* name, const void** data, int64_t* count, int* elem_bytes);
int64_t tipk_host_plan_scalar(const tipk_host_plan* plan, const char* name);
void tipk_host_plan_free(tipk_host_plan* plan);

/* 10d. The whole encoder behind one handle: FMEncoder.forward (src/layers.py:520-550, identity protein and drug features) and its
 *     autograd as the fused schedule of tip_amd/encoder.py `_EncoderStep` -- 8 + 8 launches, the same kernels with the same
 *     arguments in the same order (bit-identical results).  tip_amd/csrc/tipk_encoder.hip.
 *     tipk_encoder_build (allocates and synchronises, like tipk_graph_build): the graphs as the reference holds them, idx_bytes 4 | 8
 *         for all of them, on the device or on the host -- pp_index [2][n_pp_edges] (pp_train_indices), dp_index [2][n_dp_edges]
 *         (dp_edge_index: proteins 0 .. n_prot - 1, drugs n_prot .. n_prot + n_drug - 1), dd_index [2][n_dd_edges] (dd_train_idx)
 *         with dd_range [n_rel][2] (dd_train_range: consecutive blocks covering the edge list).  The P-P encoder is the reference's
 *         PPEncoder(n_prot): GCNConv(n_prot, 32) -> GCNConv(32, 16).  Every plan is built here, once.  TIPK_EINVAL for NULL,
 *         negative or inconsistent arguments (ids out of range, ranges that do not tile the edge list, add with n_embed !=
 *         prot_drug_dim); TIPK_EUNSUPPORTED where the fused kernels do not take the shape (the conditions of encoder.py
 *         `usable`: more than 1 024 drugs, n_hid1 != 32, widths or base counts a `*_supported` query refuses, a P -> D edge that
 *         starts at a drug, every protein a P -> D source, no P -> D edge that ends at a drug, no relation or no D-D edge) -- there
 *         is no other route behind the handle.
 *         Contracts pinned by tests/test_gpu_encoder_step_edges.py on the edge graphs of tests/encoder_cases.py (empty and one-edge
 *         relations, drugs without targets or in-edges, a hub, duplicate triples, a dense and a one-edge D-D graph, node counts that
 *         are no multiple of a tile, 1 024 drugs, the last n_rel of one LDS column block): z and all twelve gradients within
 *         k 2^-24 A of fp64 elementwise; the bits of `_EncoderStep` for lin_layout 0 | 1 and idx_bytes 4 | 8; d_norm = NULL = a
 *         tensor of ones; flags 0 = TIPK_ENCODER_FROM_FWD; TIPK_EUNSUPPORTED with a NULL handle exactly where `usable` is False.
 *     tipk_encoder_workspace_bytes: size of the caller-owned workspace (16-byte aligned).  It holds what the backward pass reads
 *         (conv outputs, x0, x1, the P -> D mean, both layers' pair cells and node-major XB, one pair-gradient table per layer) and
 *         the scratch of both passes.  tipk_encoder_workspace_init (one hipMemsetAsync on `stream`, capturable) prepares a workspace
 *         before its first use: the passes read parts of it as zeros (unlinked cells, XB padding, unused gradient rows) and keep them
 *         at zero.  One workspace per handle in flight; two handles with their own workspaces on two streams share nothing mutable.
 *     tipk_encoder_fwd: z_out [n_drug x n_hid2] (ldz = n_hid2) = the encoder output.  Parameters (tipk_encoder_params) in the
 *         reference's state_dict shapes, contiguous; the two GCN weights [out, in] as row-major storage (lin_layout 0: two launches
 *         more forward, two more backward -- transposes) or stored transposed, [in, out] in memory (lin_layout 1: how this
 *         package's modules keep them; the 16-launch schedule).  d_norm [n_drug] (nullable = 1).  x_drug must be NULL (identity drug
 *         features: x_drug @ embed = embed); dense features: TIPK_EUNSUPPORTED.
 *     tipk_encoder_bwd: from grad_z [n_drug x n_hid2] (ld_g = n_hid2) every parameter gradient in the parameter's own shape and
 *         lin_layout (overwritten; grads->embed is also the gradient of the identity drug features, g_x_drug must be NULL).
 *         flags TIPK_ENCODER_FROM_FWD: the workspace still holds what tipk_encoder_fwd with THESE parameters left in it (the
 *         semantics of TIPK_RGCN_WORKSPACE_FROM_FWD); flags 0 recomputes XB and the pair cells first (always safe, 3 launches more).
 *     fwd / bwd never allocate, never synchronise and return a status for every failure (no C++ exception crosses the ABI):
 *     both can be captured into a hipGraph. */
#define TIPK_ENCODER_FROM_FWD 1
typedef struct tipk_encoder tipk_encoder;
typedef struct tipk_encoder_dims {
    int n_embed, prot_drug_dim, n_hid1, n_hid2, num_base;
    int cat;                                   /* 1: mod 'cat', 0: mod 'add' */
} tipk_encoder_dims;
typedef struct tipk_encoder_params {
    const float* embed;                        /* embed                      [n_drug x n_embed] */
    const float* pp_w1; const float* pp_b1;    /* pp_encoder.conv1.lin.weight [32 x n_prot], .bias [32] */
    const float* pp_w2; const float* pp_b2;    /* pp_encoder.conv2.lin.weight [16 x 32], .bias [16] */
    const float* hgcn_w;                       /* hgcn.weight                [16 x prot_drug_dim] */
    const float* basis1; const float* att1; const float* root1;   /* rgcn1: [num_base x d_in x n_hid1], [n_rel x num_base], [d_in x n_hid1] */
    const float* basis2; const float* att2; const float* root2;   /* rgcn2: [num_base x n_hid1 x n_hid2], [n_rel x num_base], [n_hid1 x n_hid2] */
    int lin_layout;                            /* 0: the GCN weights row-major [out, in]; 1: stored [in, out] */
} tipk_encoder_params;
typedef struct tipk_encoder_grads {            /* the same tensors, written (GCN weights in the params' lin_layout) */
    float* embed; float* pp_w1; float* pp_b1; float* pp_w2; float* pp_b2; float* hgcn_w;
    float* basis1; float* att1; float* root1; float* basis2; float* att2; float* root2;
} tipk_encoder_grads;
int tipk_encoder_build(const void* pp_index, int64_t n_pp_edges, const void* dp_index, int64_t n_dp_edges, const void* dd_index,
                       int64_t n_dd_edges, const void* dd_range, int64_t n_rel, int idx_bytes, int64_t n_prot, int64_t n_drug,
                       const tipk_encoder_dims* dims, tipk_encoder** enc_out);
int64_t tipk_encoder_workspace_bytes(const tipk_encoder* enc);
int tipk_encoder_workspace_init(const tipk_encoder* enc, void* workspace, int64_t workspace_bytes, tipk_stream_t stream);
int tipk_encoder_fwd(const tipk_encoder* enc, const tipk_encoder_params* params, const float* x_drug /* must be NULL */, int64_t ld_x,
                     const float* d_norm /* nullable */, float* z_out, int64_t ldz, void* workspace, int64_t workspace_bytes,
                     tipk_stream_t stream);
int tipk_encoder_bwd(const tipk_encoder* enc, const tipk_encoder_params* params, const float* x_drug /* must be NULL */, int64_t ld_x,
                     const float* d_norm /* nullable */, const float* grad_z, int64_t ld_g, tipk_encoder_grads* grads,
                     float* g_x_drug /* must be NULL */, int64_t ld_gx, int flags, void* workspace, int64_t workspace_bytes,
                     tipk_stream_t stream);
int tipk_encoder_destroy(tipk_encoder* enc);
/* The encoder's plans that were built only in Python before, as host plans (section 10c; tests/test_host_encoder_plans.py):
 *   tipk_plan_hier_csr   layers.py `hier_graph` pd_csr -- arrays "fwd_ptr", "fwd_src", "scale" (float), "fwd_wg" ([n][2] =
 *                        `drug_workgroups`), "fwd_order", "t_ptr", "t_dst", "t_w" (float), "t_wg" (`deal_rows_by_edges` with the
 *                        given limits: tipk_pd_stage_bwd_limits); scalar "n_src".  dst in the concatenated node space.
 *   tipk_plan_gcn_norm   layers.py `gcn_norm_graph(edge_index, n_nodes, d=d, rows=rows)` (rows ascending, nullable = all) as the module
 *                        builds it on the DEVICE: deg^-1/2 correctly rounded (torch's device pow(-0.5); its CPU pow rounds twice).  The
 *                        grouped gather plans under "fwd." and "bwd." ("row_id", "edge_w", "items", "perm"; "n_items", "group_slots"). */
int tipk_plan_hier_csr(const int64_t* src, const int64_t* dst, int64_t n_edges, int64_t n_all, int64_t n_source, int64_t n_table,
                       int max_rows, int max_edges, tipk_host_plan** plan_out);
int tipk_plan_gcn_norm(const int64_t* src, const int64_t* dst, int64_t n_edges, int64_t n_nodes, const int64_t* rows /* nullable */,
                       int64_t n_rows, int d, tipk_host_plan** plan_out);

#ifdef __cplusplus
}
#endif
#endif /* TIPK_H */
