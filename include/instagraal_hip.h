/*
 * instagraal_hip.h -- C ABI of the MI355X-native per-move scoring path of instaGRAAL.
 *
 * The reference has no FFI of its own for this path: its Python reaches the GPU only
 * through pycuda (cuda_lib_gl_single.py, "CL").  This library replaces that layer --
 *   pycuda.compiler.SourceModule(...).get_function(name)   CL:1521-1600
 *   gpuarray / mem_alloc / memcpy_htod / memcpy_dtoh         CL:321-424, 551-646
 *   GPUStruct (struct of 17 int*)                            gpustruct.py:8-186
 * -- with a flat C ABI: one opaque handle per sampler, library-owned device memory,
 * caller-owned host memory, int return codes (0 = ok, <0 = error; text via
 * ig_last_error()).  No exceptions, callbacks or torch types cross the boundary.
 * A handle is not thread-safe; distinct handles are independent.
 * Unless stated otherwise a call returns after its work is complete (synchronous).
 *
 * Fragment state is exchanged as int32 soa[17][N] in the member order of
 * kernel_sparse_adapt.cu:40-58 ("KA"):
 *   pos sub_pos id_c start_bp len_bp sub_len circ id prev next l_cont sub_l_cont
 *   l_cont_bp ori rep activ id_d
 */
#ifndef INSTAGRAAL_HIP_H
#define INSTAGRAAL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IG_N_TMP_STRUCT 24 /* candidate mutation slots per (frag, candidate) pair, CL:192-194 */
#define IG_MAX_CANDIDATES 16
#define IG_N_INSERT_BLOCKS 6 /* CL:192 */

typedef struct ig_ctx ig_ctx;

/* outcome of one move: the 6-tuple of sampler.step_sampler (CL:1458-1465) + diagnostics */
typedef struct ig_move_result {
    double o;            /* score of the applied candidate = new likelihood_t (CL:1454-1457) */
    double dist;         /* dist_inter_genome (CL:665-716) */
    double mean_len;     /* mean_length_contigs (CL:2742), float32 value widened */
    int32_t op_sampled;  /* 0..23 */
    int32_t id_f_sampled;/* partner fragment of the applied candidate */
    int32_t n_contigs;
    int32_t n_candidates;
    int64_t n_slice;     /* sum over candidates of sliced contacts S_c (CL:1043) */
    int64_t n_evals;     /* sum over candidates of S_c * (n_uniq + 1) term evaluations */
    int64_t bytes_min;   /* compulsory-traffic model B_min of this move */
    int32_t error;       /* 0, or a device-side consistency failure code */
    int32_t pad;         /* 0 in every record a caller sees (inside the library: 1 = the one-move launches found the move's lists too long
                          * for the slice pool and applied nothing; the entry point grows the pool and repeats the move) */
} ig_move_result;

/* ---- lifetime --------------------------------------------------------- */
int ig_create(int device_id, ig_ctx** out);
void ig_destroy(ig_ctx* ctx);
const char* ig_last_error(void);
int ig_sync(ig_ctx* ctx);
/* use an existing hipStream_t (e.g. torch's current stream); NULL = library-owned stream */
int ig_set_stream(ig_ctx* ctx, void* hip_stream);

/* ---- problem upload (replaces sparse_data_2_gpu CL:551-646, create_gpu_struct CL:429-549) */
/* level-(L-1) contacts: strict upper triangle COO, row-major sorted, as CL:592-615 uploads them.
 * rank/world: contact shard of this handle (rows r with r % world == rank); (0,1) = all. */
int ig_upload_contacts(ig_ctx* ctx, const int32_t* row, const int32_t* col, const int32_t* cnt, int64_t Z, int32_t M,
                       int32_t rank, int32_t world);
/* np_sub_frags_2_frags: M x float4 (parent bin, watson kb, crick kb, index in bin), simu_single.py:701-717 */
int ig_upload_subfrag_table(ig_ctx* ctx, const float* xyzw, int32_t M);
int ig_upload_state(ig_ctx* ctx, const int32_t* soa17, int32_t N);
/* contig ids are returned renumbered exactly as modify_gl_cuda_buffer leaves them (CL:2715-2881) */
int ig_download_state(ig_ctx* ctx, int32_t* soa17);
/* which: 0 = param_simu, 1 = param_simu_test (CL:2343-2349, 3019-3023); p in KA:91-100 order */
int ig_set_params(ig_ctx* ctx, const float p[8], float mean_subfrag_kb, int which);
/* list_bounds (CL:417-422) and max_bounds_insert (CL:418-420) */
int ig_set_insert_config(ig_ctx* ctx, const int32_t list_bounds[IG_N_INSERT_BLOCKS], int32_t max_bounds_insert);
/* initial prev/next/orientable for the genome distance (CL:269-276); blacklist may be NULL */
int ig_set_initial_genome(ig_ctx* ctx, const int32_t* init_prev, const int32_t* init_next, const int32_t* orientable,
                          const int32_t* blacklisted, int32_t n_blacklisted);

/* ---- likelihood (evaluate_likelihood_sparse KA:4374-4488, eval_likelihood_on_zero KA:3850-3917) */
/* nz, z: the two scalars eval_likelihood()/approx_single_likelihood_on_zeros() leave behind
 * (CL:1245-1292, 718-760).  which_params as ig_set_params.  use_prev_tables != 0 evaluates on the
 * coordinates of the state BEFORE the last applied move (what eval_likelihood_4_nuisance sees,
 * CL:1296-1344, quirk Q12).  limbs (may be NULL): exact sums {nz_hi, nz_lo, z_hi, z_lo, n_intra}. */
int ig_full_likelihood(ig_ctx* ctx, int which_params, int use_prev_tables, double* nz, double* z, int64_t* limbs5);

/* ---- the move (step_sampler CL:1401-1465) ------------------------------ */
/* scores: C x 24 doubles laid out as all_scores (CL:1414, 1431); slots that are not scored are 0. */
int ig_score_move(ig_ctx* ctx, int32_t frag_a, const int32_t* cands, int32_t C, double* scores);
/* re-materialise (frag_a, frag_b, op) into the live state (test_copy_struct CL:2094-2151) */
int ig_apply(ig_ctx* ctx, int32_t frag_a, int32_t frag_b, int32_t op);
/* score + device argmax (CL:1435-1446) + apply + bookkeeping, one small D2H */
int ig_step(ig_ctx* ctx, int32_t frag_a, const int32_t* cands, int32_t C, ig_move_result* out, double* scores_or_null);
/* n_moves consecutive moves (the reference's inner loop over step_sampler calls, main.py full_em / CL:1401-1465).
 * cands: n_moves x max_c, -1 padded.  results: n_moves entries.
 * Moves are scored W at a time against the same state ("speculative batches": candidate draws do not depend on the
 * genome) and committed in order on the device; a move whose contigs an earlier move of its batch modified is
 * re-scored in the next batch, so the results are identical to n_moves calls of ig_step for every W. */
int ig_step_batch(ig_ctx* ctx, int32_t n_moves, const int32_t* frags, const int32_t* cands, int32_t max_c,
                  ig_move_result* results);
/* ---- the candidate draw (step 1 of step_sampler, CL:1403-1408: return_neighbours CL:3103-3141, candidates.sort()) ----
 * Host code.  The reference draws with numpy's global legacy generator -- np.random.choice(xk, k, p=pk, replace=False), or
 * np.random.choice(n_frags, k, replace=False) for a bin without hetero contacts -- and everything stochastic that follows
 * continues that stream, so the draw is restated on a COPY of the MT19937 state: the caller passes key[624] and pos from
 * np.random.get_state() and puts them back with set_state() (same lists, same generator state as numpy: tests/).
 * Distributions (setup_distri_frags, CL:3053-3101): CSR over the level-L bins, bin i -> partners xk[indptr[i]..indptr[i+1])
 * with float32 probabilities pk; an empty row = no hetero contact (the uniform draw).  Lists come out sorted, without the
 * focal bin (quirk Q13) and without blacklisted bins, -1 padded to n_neighbours. */
typedef struct ig_neighbours ig_neighbours;
int ig_neighbours_create(const int64_t* indptr, const int32_t* xk, const float* pk, int32_t n_frags, const int32_t* blacklisted,
                         int32_t n_blacklisted, ig_neighbours** out);
void ig_neighbours_destroy(ig_neighbours* nb);
int ig_neighbours_draw(ig_neighbours* nb, uint32_t* mt_key624, int32_t* mt_pos, const int32_t* frags, int32_t n_moves,
                       int32_t n_neighbours, int32_t* cands_out);
/* the same for a run of moves with nuisance sampling (instagraal.py:217-262, cycles > 4): per move the neighbour draw, then the
 * three draws of step_nuisance_parameters (CL:2976-3028): choice(4), the STANDARD normal behind normal(0, sigma) -- numpy's
 * legacy polar method with its one-value cache (has_gauss, gauss of get_state()) --, rand().  skip_normal_3: no normal is
 * drawn for modifier 3 (the reference's branch for a non-positive sigma of the trans level). */
int ig_neighbours_draw_nuisance(ig_neighbours* nb, uint32_t* mt_key624, int32_t* mt_pos, int32_t* has_gauss, double* gauss,
                                const int32_t* frags, int32_t n_moves, int32_t n_neighbours, int32_t skip_normal_3, int32_t* cands_out,
                                int32_t* id_modif_out, double* normal_out, double* uniform_out);
/* ONE complete step_sampler call (CL:1401-1465) as the reference's loop makes it (instagraal.py:221-228), candidate draw of
 * return_neighbours (CL:3103-3141) included: nb != NULL draws cands[0 .. n_neighbours) (-1 padded, *n_cands = the list's length) on
 * numpy's MT19937 state as ig_neighbours_draw does; nb == NULL scores the caller's cands[0 .. *n_cands).  Same results as ig_step,
 * less around them: the lists and the results travel through mapped host memory instead of five copies, and the move is decided
 * and applied by the batch path's fused commit kernel (a batch of one) instead of the five kernels of the one-move tail.
 * scores_or_null == NULL (the reference's loop reads all_scores nowhere outside step_sampler, CL:1414-1454): the move may be scored
 * in two tiers like a wider batch -- every column through the float screen, the exact kernel for the columns that can still win.
 * IG_STEP_DRAW_FAST=0: ig_step's way. */
int ig_step_draw(ig_ctx* ctx, ig_neighbours* nb, uint32_t* mt_key624, int32_t* mt_pos, int32_t frag_a, int32_t n_neighbours,
                 int32_t* cands, int32_t* n_cands, ig_move_result* out, double* scores_or_null);
/* n_moves complete step_sampler calls: draw (on a host thread, ahead of the launches) + ig_step_batch.  cands_out
 * [n_moves x n_neighbours] receives the drawn lists; the generator state is advanced past all n_moves draws. */
int ig_step_batch_draw(ig_ctx* ctx, ig_neighbours* nb, uint32_t* mt_key624, int32_t* mt_pos, int32_t n_moves, const int32_t* frags,
                       int32_t n_neighbours, int32_t* cands_out, ig_move_result* results);
/* The same in steps, for a caller that splits the slots of a batch over several GPUs (one process per GPU, every rank
 * holds the full problem): upload the lists once; per batch every rank builds all W candidate-genome sets but slices and
 * scores only slots [slot_begin, slot_end); the slot-major score records (ig_batch_records: one device buffer, a fixed
 * number of bytes per slot) are all-gathered by the caller; then every rank commits the batch -- identical integer
 * inputs, identical decisions, no further communication.  W <= max_w <= 64. */
int ig_batch_max_width(ig_ctx* ctx, int32_t max_c); /* largest W whose work buffers fit (<= 64; the per-slot window arrays are strided by 3 x the longest contig: ~12 MB per slot at 50 k bins in 1 000 contigs, gigabytes late in an assembly) */
int ig_batch_upload(ig_ctx* ctx, int32_t n_moves, const int32_t* frags, const int32_t* cands, int32_t max_c, int32_t max_w);
int ig_batch_score(ig_ctx* ctx, int32_t move0, int32_t W, int32_t slot_begin, int32_t slot_end); /* asynchronous */
int ig_batch_records(ig_ctx* ctx, void** records, int64_t* bytes_per_slot); /* slot w: records + w * bytes_per_slot */
int ig_batch_commit(ig_ctx* ctx, int32_t move0, int32_t W, int32_t* n_committed); /* moves move0 .. move0+n_committed-1 are done */
int ig_batch_results(ig_ctx* ctx, int32_t n_moves, ig_move_result* results);
int ig_set_batch_width(int w);                        /* W in 1..64 (default 24, env IG_BATCH_W); 1 = no speculation */
/* The WINDOW rule of ig_step_batch / ig_step_batch_draw (round 5): the scored slots of the moves ahead stay scored from launch to launch
 * while no contig they read is written; a launch re-scores the stale ones and fills the window up; decisions strictly in order, results
 * those of one move at a time (CL:1401-1465).  w = 0: off (every launch scores a fresh batch of ig_set_batch_width slots and drops what
 * lies behind its first conflict: rounds 1 - 4); w in 2..64: slots of the window (default 48, env IG_WINDOW). */
int ig_set_window(int w);
int ig_batch_stats(ig_ctx* ctx, int64_t out4[4]);     /* {batches, moves committed in-batch, one-move tails, predicted deltas used} */
/* {contacts in the CSR rows the slice kernel walked (every touched contig of a move slot once), contacts in the rows a walk per
 * candidate would have read} since the handle was created */
int ig_slice_walk_stats(ig_ctx* ctx, int64_t out2[2]);
int ig_scratch_bytes(ig_ctx* ctx, int64_t out3[3]);   /* move buffers: {per-window arrays, slice pool, per-slot records and lists} */

/* ---- a move and the nuisance step behind it, in flight together (instagraal.py:217-262 for cycles > 4: step_sampler, then
 * step_nuisance_parameters CL:2961-3051) ----------------------------------
 * The nuisance step evaluates the full likelihood under its test parameters on the coordinates of the state BEFORE the move
 * just applied (eval_likelihood_4_nuisance CL:1296-1344, quirk Q12) and needs only that move's score besides: its pass over
 * all contacts runs next to the move.  ig_nuis_begin: asynchronous -- the move (score + apply) and, on a second stream, the
 * pass under p_test (KA:91-100 order).  ig_nuis_end: waits for both; nz_test / z_test as ig_full_likelihood.  ig_nuis_accept:
 * the test parameters of the last step become param_simu (maintained sums recomputed under them, CL:3032-3036). */
int ig_nuis_begin(ig_ctx* ctx, int32_t frag_a, const int32_t* cands, int32_t C, const float p_test[8], float mean_subfrag_kb);
int ig_nuis_end(ig_ctx* ctx, ig_move_result* out, double* nz_test, double* z_test, int64_t* limbs5);
int ig_nuis_accept(ig_ctx* ctx);
/* The same for a RUN of (move, nuisance step) pairs -- the loop of instagraal.py:217-262 itself.  A rejected step changes
 * nothing a move reads, so the moves behind it are scored ahead, in batches (width: env IG_NUIS_W, default: follows the run
 * lengths, at most IG_NUIS_WMAX = 24): ig_nuis_run_begin uploads the lists of the run (as ig_batch_upload);
 * ig_nuis_step_begin(move), move = 0, 1, ... in order: asynchronous -- the step's pass under p_test and the decision + apply
 * of that ONE move from the batch it was scored in (a batch starting at `move` is scored first when there is none: first
 * step, after an accepted step, after a conflict with an earlier move of the batch, batch used up); ig_nuis_end /
 * ig_nuis_accept as above.  Results as one move and one step at a time.  Any other call that runs moves or changes state or
 * param_simu ends the run. */
int ig_links_inverse(ig_ctx* ctx); /* 1: speculative batches (ig_step_batch with W > 1, ig_batch_*, ig_nuis_run_begin) are available for this initial genome */
int ig_set_nuis_width(int w); /* moves scored ahead per launch: 0 = follow the run lengths (default, env IG_NUIS_W); results do not depend on it */
int ig_nuis_run_begin(ig_ctx* ctx, int32_t n_moves, const int32_t* frags, const int32_t* cands, int32_t max_c);
int ig_nuis_step_begin(ig_ctx* ctx, int32_t move, const float p_test[8], float mean_subfrag_kb);
/* ig_nuis_end + the acceptance test (CL:3026-3036: exp((L_test - L_move) / temperature) >= u) + ig_nuis_accept + the next
 * move's ig_nuis_step_begin (test parameters for both outcomes supplied) in one call; *accepted = 0 / 1, or 2: a close call
 * (within 1e-9 relative), nothing decided or enqueued, the caller does it with its own exp(). */
int ig_nuis_step_next(ig_ctx* ctx, double temperature, double u, const float p_next_rejected[8], const float p_next_accepted[8],
                      float mean_subfrag_kb, int32_t has_next, ig_move_result* out, double* nz_test, double* z_test, int32_t* accepted);
/* The steps of a run decide their Metropolis test (CL:3026-3036) from a SCREENED pass where they can: the change of the
 * likelihood between the model's and the test parameters, term by term in float with a rigorous bound
 * (csrc/ig_kernels_nuis.cuh); a step whose whole interval lies below T ln u is rejected without the exact pass (its *nz_test is
 * then the interval's midpoint: eval_likelihood_4_nuisance's value is only read inside the method, CL:3023-3036), every other
 * step runs the exact pass as well.  0 = the exact pass on every step (env IG_NUIS_SCREEN); env IG_NUIS_SCREEN_VERIFY=1: both
 * on every step, the bound checked. */
int ig_set_nuis_screen(int on);
/* The screened pass has two tiers.  The first reads no contact at all: the same change of the likelihood from a histogram of the
 * cis contacts over log2 of their distance (in which the term's exponent is piecewise linear), kept up to date by the moves that
 * change the genome, with its own rigorous bound; the pass over the contacts runs only where that interval does not decide
 * (csrc/ig_kernels_nuis.cuh, "tier 0").  1 (default): where it pays -- a cost model on the host (contacts, contigs, share of the
 * moves that change the genome) switches it off where few long contigs make the walks dearer than the pass; 2: always; 0 = start
 * with the pass over the contacts (env IG_NUIS_HIST); IG_NUIS_SCREEN_VERIFY=1 checks both tiers against the exact pass on every
 * step. */
int ig_set_nuis_hist(int on);
/* Chains: the pairs move .. move + n_sets - 1 of a run, as far as the device can take them WITHOUT the host (csrc/ig_common.cuh,
 * ChainIn): per segment the Metropolis intervals of the next 8 steps' test sets from the histogram tier in one launch, then one decide
 * wave that takes the moves from the batch's score records in order and tests each step (CL:3026-3036) against its interval with
 * the live likelihood; it stops in front of the first pair that needs the host (a step that is not a certain rejection, a conflict,
 * a pending windowed winner, an overflow) -- that pair is untouched and goes through ig_nuis_step_begin / ig_nuis_step_next -- and
 * goes on behind a move that changed the genome once the histogram has followed it.  p_tests [n_sets][8] in KA:91-100 order, u /
 * temperature [n_sets]: the acceptance uniforms and temperatures of those steps (n_sets <= 64).  Asynchronous: a helper thread
 * drives the segments; ig_nuis_chain_done polls (1: ended), ig_nuis_chain_end waits: *n_done pairs completed (each a move decided
 * exactly as ig_step_batch decides it and a step rejected with the margins of ig_nuis_step_next; their records: ig_batch_results),
 * *reason: 0 sets used up, 1 test, 2 conflict, 3 pending, 4 overflow, 5 no slot scored under the model's parameters, 6 the
 * histogram tier is not in use.  ig_set_nuis_chain(0) / env IG_NUIS_CHAIN=0: the runs keep to one pair per call (and score their
 * batches without winner prediction).  Results do not depend on any of it. */
int ig_set_nuis_chain(int on);
int ig_nuis_chain_begin(ig_ctx* ctx, int32_t move, int32_t n_sets, const float* p_tests, const double* u, const double* temperature,
                        float mean_subfrag_kb);
int ig_nuis_chain_done(ig_ctx* ctx);
int ig_nuis_chain_end(ig_ctx* ctx, int32_t* n_done, int32_t* reason);
/* *accepted = 3 from ig_nuis_step_next: the step was ACCEPTED from the screened interval alone (every L_test in it gives a ratio
 * above u); its exact pass -- the promotion of the maintained sum needs it, the decision does not -- runs behind the decision, next
 * to the re-scoring of the moves ahead; *nz_test was the interval's midpoint.  The exact value (what eval_likelihood_4_nuisance
 * returns, CL:1296-1344, and likelihood_t becomes, CL:3036): here, any time before the next step is accepted that way. */
int ig_nuis_exact_result(ig_ctx* ctx, double* nz_test);

/* ---- bookkeeping -------------------------------------------------------- */
int ig_renumber_contigs(ig_ctx* ctx, int32_t* n_contigs, float* mean_len, int32_t* max_id); /* CL:2715-2881 */
int ig_bomb(ig_ctx* ctx, const int32_t* shuffle);                                            /* CL:1925-1948 */
int ig_genome_distance(ig_ctx* ctx, double* d);                                              /* CL:665-716 */
int ig_get_valid_insert(ig_ctx* ctx, int32_t out12[12]); /* gpu_list_valid_insert, stale-flag state (Q4) */

/* ---- the contact map of the current genome (display_current_matrix CL:2555-2605) ----
 * The reference densifies sparse_matrix + sparse_matrix.T and indexes it by full_order_high, the sub-fragments in the order of the
 * genome (CL:2563-2585, 2598-2599).  Here: the same ORDER, and the matrix under it as a binned image built from the device copy
 * of the contacts, of bounded size whatever M is.
 * Order: contigs by ascending contig id as ig_download_state returns it (the reference walks np.unique of its ids), a contig only if
 * every one of its bins has activ == 1 (CL:2571); inside a contig the bins by pos, inside a bin the sub-fragments in table order,
 * reversed when ori == -1 (CL:2576-2585).  order_M: caller-owned, M entries of room; order_M[r] = the sub-fragment at position r for
 * r < *n_placed = T.
 * Image: bin = max(1, ceil(T / max_side)) positions per pixel, side = ceil(T / bin), pixel of position r = r / bin;
 * image[pi * side + pj] = sum of the counts of the uploaded contacts between pixels pi and pj, both ways round (a contact inside one
 * pixel counts twice there): with max_side >= T the reference's matrix entry for entry, EXCEPT its diagonal -- ig_upload_contacts
 * takes the strict upper triangle, so self-contacts (twice the diagonal of the input matrix in the reference's picture) are not in
 * the image; a caller that has them adds them (instagraal_amd.sampler.contact_map does).  64-bit integer sums: exact, and the same
 * from run to run.  image: caller-owned, image_capacity entries; *side and *bin are set first, then image_capacity < side * side is
 * an error and nothing is written.
 * Both calls read the CURRENT coordinates and change nothing a move reads (no state, tables, maintained sums, slice pools, window
 * slots): moves scored ahead stay valid.  Synchronous.  They do NOT end a nuisance step or a chain in flight: between ig_nuis_begin /
 * ig_nuis_step_begin and ig_nuis_end, and between ig_nuis_chain_begin and ig_nuis_chain_end, they return an error.
 * A sharded handle (ig_set_shard) adds its shard's rows only: the partial images of all ranks sum to the image. */
int ig_contact_map_order(ig_ctx* ctx, int32_t* order_M, int32_t* n_placed);
int ig_contact_map(ig_ctx* ctx, int32_t max_side, int64_t* image, int64_t image_capacity, int32_t* side, int32_t* bin);

/* ---- the distance law P(s) of the current genome (no reference counterpart; the rule: instagraal_amd/distance_law.py) ---------
 * edges: n_edges ascending finite floats (kb), 2 <= n_edges <= 4097; bin b holds the separations edges[b] <= s < edges[b + 1].
 * A pair of sub-fragments of one placed contig (placed as for the contact map: every bin active) that is not a ring has
 * s = fabsf(dist_i - dist_j) on the current coordinate table, in float.  observed[b] (n_edges - 1 entries): sum of the counts of the
 * uploaded contacts between such pairs; pairs[b]: the number of such pairs, with or without a contact (NULL: the pairs pass is
 * skipped and the pair scalars are -1).
 * scalars: {0 out_of_range_observed, 1 out_of_range_pairs (s < edges[0] or s >= edges[n_edges - 1]), 2 trans_observed,
 * 3 trans_pairs (both ends placed, different contigs; the pairs from the sub-fragment counts: T (T - 1) / 2 - placed_pairs),
 * 4 ring_observed, 5 ring_pairs (inside a ring contig: two separations, left out of the law), 6 unplaced_observed (an end in a
 * contig that is not placed), 7 placed_pairs = sum over the placed contigs of M_c (M_c - 1) / 2}.
 * By construction: sum(observed) + scalars[0] + [2] + [4] + [6] = sum of all counts; sum(pairs) + scalars[1] + [5] = scalars[7].
 * 64-bit integer sums: exact, the same from run to run.  Guards and effects as ig_contact_map: reads the CURRENT coordinates, changes
 * nothing a move reads, synchronous, an error while a nuisance step or a chain is in flight.  A sharded handle (ig_set_shard) adds its
 * shard's rows to observed and the observed scalars -- the ranks' results sum to the whole -- and computes the pairs whole. */
int ig_distance_law(ig_ctx* ctx, const float* edges, int32_t n_edges, int64_t* observed, int64_t* pairs, int64_t scalars[8]);

/* ---- the junction support profile of the current genome (no reference counterpart; the rule: instagraal_amd/junction_profile.py) --
 * Positions: the contact map's -- the placed sub-fragments in the order of ig_contact_map_order, 0 .. T - 1.  Junction j, 1 <= j <= T - 1,
 * lies between the positions j - 1 and j; the arrays have T entries indexed by j, entry 0 is 0.  window: 1 .. 1024 positions.
 * observed[j]: sum of the counts of the uploaded contacts with both ends placed in one contig that is not a ring, at positions
 * pa < pb with pb - pa <= window and pa < j <= pb.  pairs[j]: the number of pairs of positions (i, k) of that contig with
 * i < j <= k and k - i <= window, with or without a contact.  expected_q[j]: the sum over the same pairs of the model's value at
 * s = fabsf(dist_i - dist_k) under the parameter set moves are scored under (set 0) -- ig_detmath.h's Rippe curve, quantised as every
 * exact sum of the library is -- in units of 2^-32.
 * At a contig boundary and inside a ring all three are 0.  pairs and expected_q may BOTH be NULL: the model pass is skipped.
 * scalars: {0 in_window_observed, 1 beyond_window_observed (same linear contig, pb - pa > window), 2 trans_observed, 3 ring_observed,
 * 4 unplaced_observed, 5 internal_junctions (both positions in one contig that is not a ring), 6 spanned_observed = sum(observed),
 * 7 unused (0)}.  By construction scalars[0] + .. + [4] = sum of all counts and sum(observed) = sum of count * (pb - pa) over the
 * in-window contacts.  64-bit integer sums: exact, the same from run to run, whatever the launch shapes.
 * capacity: entries of room in each array; *n_placed = T is set first, then capacity < T is an error and nothing is written.
 * An error too, with nothing written: a parameter set under which the largest quantised model value times window (window + 1) / 2
 * reaches 2^62 ("model value too large for this window": the sum could overflow).
 * Guards and effects as ig_contact_map: reads the CURRENT coordinates, changes nothing a move reads, synchronous, an error while a
 * nuisance step or a chain is in flight.  A sharded handle (ig_set_shard) adds its shard's rows to observed and the observed scalars
 * -- the ranks' results sum to the whole -- and computes pairs and expected_q whole. */
int ig_junction_profile(ig_ctx* ctx, int32_t window, int64_t* observed, int64_t* pairs, int64_t* expected_q, int64_t capacity,
                        int32_t* n_placed, int64_t scalars[8]);

/* ---- the contacts in the coordinates of the current genome (no reference counterpart on the device: the reference lifts the raw
 * pairs over on the host; the rule: instagraal_amd/assembly_contacts.py) ---------------------------------------------------------
 * Every uploaded contact (row, col, count) re-indexed to UNITS of the genome order and sorted: level 0, a unit is a position of
 * ig_contact_map_order (n_units = T); level 1, a unit is a placed bin, numbered in genome order (the sub-fragments of a bin are
 * neighbours in the order: the unit changes where the parent bin does).  A contact with both ends placed becomes the entry
 * (lo, hi) = (min, max) of its ends' units; level 1 sums the counts of equal entries, entries with lo == hi (two sub-fragments of
 * one bin) included.  The result is the CSR form of the upper triangle: rowptr[n_units + 1], and per entry the column hi (strictly
 * ascending inside a row) and the count as a 64-bit sum -- the arrays of the rule byte for byte, whatever the launch shapes and
 * the order in which atomics land, and the same from run to run.
 * scalars: {0 entries_in (contacts of this handle's shard), 1 entries_kept, 2 contacts_kept (sum of their counts), 3 entries_unplaced
 * (an end in a contig that is not placed), 4 contacts_unplaced, 5 n_placed = T, 6 n_units, 7 entries_out = *n_entries}.  By
 * construction [2] + [4] = sum of all counts, the counts of the result sum to [2], and at level 0 [7] = [1].
 * ig_assembly_contacts_build leaves the result ON THE DEVICE, a snapshot: moves made afterwards do not change it.  It is released by
 * ig_assembly_contacts_release, by the next build (also one that fails: no stale result is ever visible), by ig_upload_contacts
 * and by ig_destroy.  ig_assembly_contacts_rows copies rowptr (capacity: words of room, n_units + 1 needed),
 * ig_assembly_contacts_fetch the entries first .. first + n - 1 (so that a host takes 5 10^8 entries in pieces); without a built
 * result, out of range, or with a level other than 0 and 1 they return an error and write nothing.  They serve the snapshots of
 * ig_assembly_contacts_build_units and ig_assembly_contacts_coarsen (below) as they serve one of level 1.
 * Device memory: 8 bytes per kept entry while the result lives (level 1: 12 per summed entry), 16 during a build that has long rows.
 * Guards and effects as ig_contact_map: reads the CURRENT coordinates, changes nothing a move reads, synchronous, an error while a
 * nuisance step or a chain is in flight.  A sharded handle (ig_set_shard) takes its shard's rows: the ranks' results, merged entry by
 * entry, are the whole. */
int ig_assembly_contacts_build(ig_ctx* ctx, int32_t level, int64_t* n_units, int64_t* n_entries, int64_t scalars[8]);
int ig_assembly_contacts_rows(ig_ctx* ctx, int64_t* rowptr, int64_t capacity);
int ig_assembly_contacts_fetch(ig_ctx* ctx, int64_t first, int64_t n, int32_t* col, int64_t* count);
int ig_assembly_contacts_release(ig_ctx* ctx);

/* ---- join support: which scaffold ends the contacts would link (no reference counterpart; the rule:
 * instagraal_amd/join_support.py) -----------------------------------------------------------------------------------------------
 * The junction profile for junctions that do not exist yet.  The placed contigs that are not rings are the runs k = 0 .. K - 1 of
 * ig_contact_map_order; contig k has the ENDS 2 k (its head: its first position) and 2 k + 1 (its tail).  A contact between two
 * different such contigs counts, for each of the four pairs of their ends, for the LINK (lo, hi) = (min, max) of the two end ids
 * if the separation in positions the two sub-fragments would have with those ends joined -- depth + depth + 1 -- is at most
 * `window` (1 .. 1024).  The result lists the links with at least one contact as CSR over the 2 K ends: rowptr[2 K + 1], and per link
 * the column hi (strictly ascending inside a row), observed (the sum of the counts), pairs (the position pairs within the window)
 * and expected_q (the sum over those pairs of the model's value under parameter set 0 at the separation the coordinates would give
 * with no gap between the scaffolds, quantised to 2^-32 and added as 64-bit integers) -- the arrays of the rule byte for byte,
 * whatever the launch shapes and the order in which atomics land.  model = 0 skips the model pass: no pairs, no expected_q.
 * scalars: {0 in_reach_observed (trans contacts between linear placed contigs that count for a link, each once), 1
 * out_of_reach_observed, 2 cis_observed, 3 ring_observed (an end in a ring), 4 unplaced_observed (an end in a contig that is not
 * placed; checked first, then the ring, then cis), 5 contributions (sum of count x links counted for), 6 n_contigs = K, 7 n_links}.
 * [0] + .. + [4] = the sum of all counts; the observed of the result sum to [5].  *n_ends = 2 K.
 * ig_join_support_build leaves the result ON THE DEVICE, a snapshot: moves made afterwards do not change it.  It is released by
 * ig_join_support_release, by the next build (first thing, also one that fails), by ig_upload_contacts and by ig_destroy.
 * ig_join_support_ends copies the first position and the positions of every contig k (capacity: entries of room, K needed),
 * ig_join_support_rows copies rowptr (capacity: words of room, 2 K + 1 needed), ig_join_support_fetch the links first ..
 * first + n - 1 (pairs and expected_q may both be NULL; they must be for a result built with model = 0); without a built result or
 * out of range they return an error and write nothing.
 * Device memory: 28 bytes per link while the result lives; during a build 8 bytes per (contact, link) entry -- behind a bomb up to
 * four per contact -- and as much again for long rows.  A build whose entries do not fit the free device memory fails before it
 * allocates them and names the bytes it needs; so does one whose model values could overflow the 64-bit sum ("model value too
 * large for this window").
 * Guards and effects as ig_contact_map: reads the CURRENT coordinates, changes nothing a move reads, synchronous, an error while a
 * nuisance step or a chain is in flight.  A sharded handle (ig_set_shard) takes its shard's rows: the ranks' results, merged link
 * by link (observed summed, pairs and expected_q the same on every rank that has the link), are the whole. */
int ig_join_support_build(ig_ctx* ctx, int32_t window, int32_t model, int64_t* n_ends, int64_t* n_links, int64_t scalars[8]);
int ig_join_support_ends(ig_ctx* ctx, int32_t* first_position, int32_t* n_positions, int64_t capacity); /* per contig k */
int ig_join_support_rows(ig_ctx* ctx, int64_t* rowptr, int64_t capacity);
int ig_join_support_fetch(ig_ctx* ctx, int64_t first, int64_t n, int32_t* col, int64_t* observed, int64_t* pairs, int64_t* expected_q);
int ig_join_support_release(ig_ctx* ctx);

/* ---- the expected contact map of the current genome (no reference counterpart) -------------------------------------------
 * What the model in use predicts for the pixels of ig_contact_map's image (same positions, same binning under max_side, same
 * convention: symmetric, a pair inside one pixel counted twice on the diagonal); the rule is instagraal_amd/expected_map.py.
 * Three images of side x side int64 each (image_capacity: entries of room in EACH): cis_q, the sum of the model's value under
 * parameter set 0 at s = |dist_i - dist_k| (f32), quantised as every term of the likelihood is (multiples of 2^-32), over the pairs
 * of positions i < k of one placed contig that is not a ring; cis_pairs, the number of these pairs; ring_pairs, the number of pairs
 * on a ring (they get no model value).  The trans pairs follow on the host: n_a n_b less the two counts, each worth the quantised
 * v_inter.
 * scalars: {n_placed, linear_cis_pairs, ring_pairs, max_q: the largest |quantised value| seen, tiles_evaluated, tiles_constant (both
 * 0 under the row form), 0, 0}.  *side and *bin are set before the capacity is checked.  T == 0: side = 0 and success.
 * Fails where parameters were never set, max_side < 1, a capacity is below side^2, or 2 bin^2 max(max_q, q_trans) >= 2^62 ("model
 * value too large for this pixel size").
 * Guards and effects as ig_contact_map: reads the CURRENT coordinates, changes nothing a move reads, synchronous, an error while a
 * nuisance step or a chain is in flight.  No contact is read (none need be uploaded): the result is independent of the shard
 * (ig_set_shard), whole on every rank.  Device memory: 24 bytes per pixel during the call, nothing behind it. */
int ig_expected_map(ig_ctx* ctx, int32_t max_side, int64_t* cis_q, int64_t* cis_pairs, int64_t* ring_pairs, int64_t image_capacity,
                    int32_t* side, int32_t* bin, int64_t scalars[8]);

/* ---- placement support: where the contacts say each bin belongs (no reference counterpart; the rule:
 * instagraal_amd/placement_support.py) --------------------------------------------------------------------------------------------
 * A GUEST is a placed bin of a linear contig (the runs k = 0 .. K - 1 of ig_contact_map_order, as the join support numbers them); its
 * positions are consecutive, n_positions of them.  With the guest taken out of the order, a SITE (k, u) is the gap in front of
 * offset u of contig k (u = 0: off the head, u = the contig's remaining positions: off the tail); its window is the up to `window`
 * (1 .. 1024) positions on its left and on its right, `hosts` in all.  The guest's contacts with other bins (both ends in linear placed
 * contigs) inside the two halves are *_left and *_right.  home: the site where the guest sits (contig, offset).  best: among the
 * sites with hosts >= min_hosts (1 .. 2 window) whose window is disjoint from home's (another contig, or at least 2 window sites
 * away) the one with the highest (left + right) / hosts, compared with exact integers, the lowest (contig, offset) among equals;
 * best_contig = -1: no such site has a contact.  second: the same among the sites in another contig than the best or at least
 * 2 window sites from it.  Every array has N entries (the bins) and belongs to the caller; status: 0 guest, 1 not placed, 2 on a
 * ring -- the rows of bins that are no guests are 0, their contig fields -1.  The arrays are the rule's byte for byte, whatever the
 * launch shapes, the form of the scan and the order in which atomics land.
 * scalars: {0 unplaced_observed (an end in a contig that is not placed; checked first), 1 ring_observed (then: an end on a ring), 2
 * within_bin_observed (then: both ends in one bin), 3 counted_observed, 4 entries (two per counted contact), 5 n_contigs = K, 6
 * n_guests}.  [0] + .. + [3] = the sum of all counts.
 * Device memory: during the call 8 bytes per entry and as much again for long rows, 20 bytes per summed entry, 140 bytes per bin;
 * nothing behind it (also not behind a call that fails).  A call whose entries do not fit the free device memory fails before it
 * allocates them and names the bytes it needs; so does one with 2 window sum(counts) >= 2^62 ("counts too large for this window").
 * Guards and effects as ig_contact_map: reads the CURRENT coordinates, changes nothing a move reads, synchronous, an error while a
 * nuisance step or a chain is in flight.  A sharded handle (ig_set_shard) is refused: the maximum needs the whole profile. */
int ig_placement_support(ig_ctx* ctx, int32_t window, int32_t min_hosts, int32_t* status, int32_t* contig, int32_t* offset, int32_t* n_positions,
                         int32_t* home_hosts, int32_t* best_contig, int32_t* best_offset, int32_t* best_hosts, int32_t* second_contig,
                         int32_t* second_offset, int32_t* second_hosts, int64_t* home_left, int64_t* home_right, int64_t* best_left,
                         int64_t* best_right, int64_t* second_left, int64_t* second_right, int64_t scalars[7]);

/* ---- orientation support: which segments the contacts would reverse (no reference counterpart; the rule:
 * instagraal_amd/orientation_support.py) ------------------------------------------------------------------------------------------
 * Positions: the contact map's, 0 .. T - 1 (ig_contact_map_order).  The caller gives n_seg SEGMENTS [seg_first[k], seg_last[k]] of
 * positions, ascending, disjoint, each inside one placed contig; they need not cover the order.  With n = last - first + 1 a
 * segment's ARM is m = min(n / 2, window) -- the left arm [first, first + m - 1], the right arm [last - m + 1, last] -- and its
 * FLANKS are the up to `window` (1 .. 1024) positions of its contig on either side.
 * geometry[k] = {status, arm, left_flank, right_flank}; status, the first that fits: 1 fewer than two positions, 2 on a ring, 3 both
 * flanks empty, 0 judged.  arm and flanks are 0 on a ring.  The rows of observed and expected_q of a segment that is not judged are 0.
 * observed[k] = {LL, LR, RL, RR} (arm, flank): a contact with both ends placed in one linear contig at positions pa < pb, in the
 * segments sa and sb (-1: none), sa != sb or both -1, counts its lower end for sa if sa is judged and pb - last[sa] <= window -- to LR
 * if pa is in the left arm, to RR if in the right arm -- and its upper end for sb if sb is judged and first[sb] - pa <= window -- to LL
 * if pb is in the left arm, to RL if in the right arm.  keep = LL + RR, flip = LR + RL; reversing the segment swaps LL with RL and LR
 * with RR exactly.
 * expected_q[k] = {keep, flip} (model != 0; NULL allowed iff model == 0): the sum over the m * (left_flank + right_flank) pairs (arm
 * position, flank position) of each class of the model's value at s = fabsf(dist_i - dist_k) under parameter set 0, quantised, in
 * units of 2^-32 (the junction profile's q).
 * scalars: every contact in the first class it fits {0 unplaced, 1 trans, 2 ring, 3 within_segment (sa == sb >= 0), 4 counted (a
 * quadrant took it), 5 uncounted}, then {6 entries_observed = the sum of all quadrants, 7 n_judged}.  [0] + .. + [5] = the sum of all
 * counts; [4] <= [6] <= 2 [4].  64-bit integer sums: exact, the same from run to run, whatever the launch shapes.
 * Fails, with nothing written and the handle usable: a NULL output, a window out of range, a malformed list ("segment list ..."),
 * and a parameter set under which the largest quantised model value times 2 window^2 reaches 2^62 ("model value too large for this
 * window").  n_seg == 0 is no error: every linear cis contact is uncounted.
 * Guards and effects as ig_contact_map: reads the CURRENT coordinates, changes nothing a move reads, synchronous, an error while a
 * nuisance step or a chain is in flight.  A sharded handle (ig_set_shard) adds its shard's rows to observed and the class scalars
 * -- the ranks' results sum to the whole -- and computes geometry and expected_q whole.  Device memory: 4 bytes per sub-fragment and
 * 100 bytes per segment, kept from call to call. */
int ig_orientation_support(ig_ctx* ctx, int32_t window, int32_t model, int32_t n_seg, const int32_t* seg_first, const int32_t* seg_last,
                           int32_t* geometry /*[n_seg][4]: status, arm, left_flank, right_flank*/, int64_t* observed /*[n_seg][4]*/,
                           int64_t* expected_q /*[n_seg][2], NULL allowed iff model==0*/, int64_t* scalars /*[8]*/, int32_t* n_placed);

/* ---- multi-GPU (contact shards) -------------------------- */
/* Two-phase move: partial sums over this handle's contact shard are left in a device buffer of
 * ig_partials_count() int64 values; the caller all-reduces (SUM) it across ranks, then finishes. */
int ig_set_shard(ig_ctx* ctx, int32_t rank, int32_t world); /* score rows r with r % world == rank */
int64_t ig_partials_count(ig_ctx* ctx);
void* ig_partials_device_ptr(ig_ctx* ctx);
int ig_step_begin(ig_ctx* ctx, int32_t frag_a, const int32_t* cands, int32_t C);
int ig_step_finish(ig_ctx* ctx, ig_move_result* out, double* scores_or_null);

/* ---- timing / roofline -------------------------------------------------- */
/* average duration (ms) of the named kernel over the launches since the last reset, measured
 * with hipEvents on the library's stream; name in {"score","mutate","gather","finalize","apply","post"} */
int ig_kernel_time_ms(ig_ctx* ctx, const char* name, double* avg_ms, int64_t* n_launches);
int ig_reset_timers(ig_ctx* ctx, int enable);
int ig_set_timer_sampling(ig_ctx* ctx, int every); /* hipEvent pairs around every n-th launch only (an event record costs ~6 us of idle queue) */

/* ---- debug ABI (kernel-granularity parity tests) ------------------------ */
/* evaluate the model on arrays: ex = rippe(s), exc = rippe_circ(s, s_tot), term, quantised term */
int ig_debug_eval_terms(ig_ctx* ctx, const float* s, const float* s_tot, const int32_t* ob, int64_t n, float* ex, float* exc,
                        double* term, int64_t* q);
/* candidate genome (cand index c, slot) of the last ig_score_move, as soa17 (ids internal) */
int ig_debug_candidate_state(ig_ctx* ctx, int32_t c, int32_t slot, int32_t* soa17);
/* per-(candidate, slot) exact sums of the last scored move: nz limbs, z limbs, n_intra, extract limbs, S_c */
int ig_debug_last_sums(ig_ctx* ctx, int64_t* nz_hi, int64_t* nz_lo, int64_t* z_hi, int64_t* z_lo, int64_t* n_intra,
                       int64_t* ext_hi, int64_t* ext_lo, int64_t* n_slice, int32_t* n_uniq, int32_t* uniq);
int ig_debug_tables(ig_ctx* ctx, float* dist, int32_t* id_c, float* s_tot, int32_t* pos, int32_t* len);
/* the P_z table ig_set_params built for set `which` (0 or 1): *n its length, out[0 .. min(*n, cap)) its entries */
int ig_debug_pz_table(ig_ctx* ctx, int32_t which, float* out, int32_t cap, int32_t* n);
/* maintained exact sums {nz_hi, nz_lo, z_hi, z_lo, n_intra}; {n_contigs, next_cid, chosen c, k, slot, windowed} */
int ig_debug_globals(ig_ctx* ctx, int64_t* sums5, int32_t* ints6);
int ig_debug_dbg(ig_ctx* ctx, int32_t* out8, int32_t clear); /* Glob.dbg: the eight words a device-side consistency failure leaves (tuning builds: tick counters) */
/* two-tier scoring of the batches (csrc/ig_kernels_screen.cuh): the hardware log2 / exp2 the screening bound leans on, measured
 * over their whole domain {max |v_log_f32(s) - log2 s| / (2^-23 (|result| + 1)), max |v_exp_f32(y) - 2^y| / (2^-23 2^y)};
 * and {largest |screened - exact| / bound, largest bound} of the runs under IG_SCREEN_VERIFY=1, {columns screened, columns
 * scored exactly} */
int ig_debug_transcendental_error(ig_ctx* ctx, double out2[2]);
int ig_debug_screen_stats(ig_ctx* ctx, double out6[6]); /* ..., terms screened, terms scored exactly */
/* 0 disables the reference's dropped-tail behaviour of eval_sub_likelihood (quirk Q5); default 1 */
int ig_debug_set_tail_quirk(int on);
int ig_debug_tile_trace(ig_ctx* ctx, int64_t* out4n, int64_t cap, int64_t* n_items); /* per-workgroup clocks of one from-scratch pass */
int ig_debug_nuis_wait(ig_ctx* ctx, double* seconds); /* time ig_nuis_end has waited for the device */
/* per-workgroup clocks of one screened nuisance pass under p_test (8 words per workgroup; see ig_hip.hip) and its output words */
int ig_debug_diff_trace(ig_ctx* ctx, const float p_test[8], float mean_subfrag_kb, int64_t* out8n, int64_t cap, int64_t* n, int64_t* sums8);
/* the screened nuisance pass: {steps screened, rejected from the interval alone, exact passes behind a screened one, void,
 * largest bound, largest |screened - exact| / bound seen, sum of the bounds, steps whose interval did not decide, void because of
 * {the parameter pair, a contact, a workgroup's sums, a move record that did not come from the batch commit}} */
int ig_debug_nuis_screen_stats(ig_ctx* ctx, double out12[12]);
/* its histogram tier: {evaluations, steps rejected there, accepted there, void, sum of its bounds, largest |screened - exact| / bound
 * seen, moves walked into the histogram, builds from scratch, void because of {as above}} */
int ig_debug_nuis_hist_stats(ig_ctx* ctx, double out12[12]);
/* the maintained histogram against one built from scratch (the last move of the run is walked in first): words that differ, -1: none kept */
int ig_debug_nuis_hist_check(ig_ctx* ctx, int64_t* mismatches);
/* two-tier scoring, the decide step's zero-score rule (a score of exactly 0.0 counts as "not scored", CL:1435-1440: a move whose
 * contenders hold one under the live scalars is scored again with every column exact): fault injection for the tests -- every n-th
 * move of a two-tier batch takes that path (0 = off) -- and how often a handle has taken it */
int ig_debug_set_zero_inject(int every);
int ig_debug_zero_fallbacks(ig_ctx* ctx, int64_t* fallbacks);
/* tests: the census of the decide rounds (k_decide_commit_par).  With the switch on (process-wide, default off) every round
 * adds one to the counter of the way it ended; out16 = {launches, rounds, moves kept, all four kept, end of the batch behind four
 * moves / behind fewer, cut behind a state-changing move, cut in front of a move decided under other flags, conflict / pool / grid
 * stop at position 0 / later, zero-score stop at 0 / later, pending windowed winner at 0 / later, launches that resumed a batch,
 * rounds none of these describes (always 0)}; clear = 1 zeroes the handle's counters behind the read.  Results do not depend on it. */
int ig_debug_set_round_census(int on);
int ig_debug_round_census(ig_ctx* ctx, int32_t out16[16], int32_t clear);
/* tests: moves of the one-move path (ig_step, ig_score_move, ig_apply, ig_step_begin, ig_step_batch at width 1, ig_nuis_begin) whose
 * lists did not fit the slice pool and were repeated with a larger one -- the counterpart of the batch path's re-run slots
 * (replaces nothing in the reference: its sort buffers are sized for the whole matrix, CL:1009-1069) */
int ig_debug_pool_retries(ig_ctx* ctx, int64_t* n);
/* tests: the bytes the per-window arrays of THIS handle's move buffers may take (default 64e9; bytes <= 0: the default again).  The
 * arrays are released and sized again under the new budget at the strides the present contig lengths ask for; *slots (may be NULL): the
 * move slots they hold now, 0 before any move buffers exist.  Every launch is capped by the slots held, so results do not depend on it. */
int ig_debug_window_budget(ig_ctx* ctx, double bytes, int32_t* slots);
int ig_debug_step_stats(ig_ctx* ctx, int64_t out2[2]); /* ig_step_draw: {calls that went through mapped memory, of them finished by the one-move tail} */
int ig_debug_nuis_chain_stats(ig_ctx* ctx, int64_t out10[10]); /* chains: {calls, segments, pairs completed, ends by reason [7]} */
int ig_debug_set_full_hist(int on); /* from-scratch pass: all-trans tiles from their count histograms (1, default) or contact by contact (0) */

/* the contact map's pass (zero + k_contact_map + mirror) n times under max_side, hipEvents around each: ms_n[n]; combine = 0: the
 * form with one atomic per contact end (the yardstick the wave-combined form is measured against); *image_sum (may be NULL): the
 * sum of the last image */
int ig_debug_contact_map_time(ig_ctx* ctx, int32_t max_side, int32_t combine, int32_t n, float* ms_n, int64_t* image_sum);
/* the distance law's passes n times each, hipEvents around each (zero + kernel): ms_observed_n[n] -- privatised = 1: the form with a
 * histogram per workgroup in LDS, 0: one global atomic per contact (the yardstick) -- and ms_pairs_n[n] (may be NULL: not run);
 * *checksum (may be NULL): the last observed pass's words, each weighted by its place: both forms must agree on it */
int ig_debug_distance_law_time(ig_ctx* ctx, const float* edges, int32_t n_edges, int32_t privatised, int32_t n, float* ms_observed_n,
                               float* ms_pairs_n, int64_t* checksum);
/* the junction profile's passes n times each, hipEvents around each: ms_observed_n[n] (zero + kernel) -- combine = 1: equal + ends
 * summed inside the wave first, 0: one atomic per contact end (the yardstick) --, ms_model_n[n] (may be NULL: not run) and
 * ms_scan_n[n] (may be NULL: the scan runs once, untimed); *checksum (may be NULL): the observed profile behind the last pass and
 * its five scalars, each word weighted by its place: both forms must agree on it */
int ig_debug_junction_profile_time(ig_ctx* ctx, int32_t window, int32_t combine, int32_t n, float* ms_observed_n, float* ms_model_n,
                                   float* ms_scan_n, int64_t* checksum);
/* the contacts in genome coordinates: every row of the build is sorted by the form its length picks -- up to short_max entries a
 * wave per row, up to lds_max a workgroup per row in LDS, beyond that runs of lds_max entries merged through a scratch buffer.  The
 * limits of THIS handle: 0 = the compiled default (64, 1024), a value above a form's capacity (64, 1024) counts as the capacity;
 * (1, 1) sends every row through the long form.  For the tests and the bench: the result does not depend on the limits. */
int ig_debug_assembly_contacts_limits(ig_ctx* ctx, int32_t short_max, int32_t lds_max);
/* the two passes over the contacts of THIS handle's builds: combine = 1 (the default): a run of a wave's lanes with the same row
 * issues one atomic; 0: one atomic per contact, the yardstick the combined form is measured against.  The result is the same. */
int ig_debug_assembly_contacts_combine(ig_ctx* ctx, int32_t combine);
/* the last build's work lists: {rows, entries} of the short, the lds and the long form, the runs the long rows were cut into, the
 * longest long row (rows of fewer than two entries are on no list) */
int ig_debug_assembly_contacts_forms(ig_ctx* ctx, int64_t out8[8]);
/* tests: the `activ` flag of one bin on the device (ig_upload_state refuses a state with an inactive bin, as the reference's moves
 * cannot handle one).  Only the genome order reads the flag: a contig with an inactive bin is not placed -- left out of the contact
 * map, the distance law, the junction profile and the contacts in genome coordinates, and counted there as unplaced */
int ig_debug_set_bin_active(ig_ctx* ctx, int32_t bin, int32_t active);
/* the build n times, hipEvents around each pass: ms_n[n][7] = {count, scan, scatter, sort short, sort lds, sort long, reduce (level 1)};
 * the last result stays built; *checksum (may be NULL): its rows, columns and counts, each word weighted by its place */
int ig_debug_assembly_contacts_time(ig_ctx* ctx, int32_t level, int32_t n, float* ms_n, int64_t* checksum);
/* tests: the 64-bit scan of the reports (k_scan64_totals / _tops / _apply) over caller data, unchanged: the inclusive prefix sums,
 * modulo 2^64, of the first n words of n_arrays arrays `stride` words apart (stride >= n).  in and out: n_arrays * stride words each;
 * both go to the device, the scan runs from one buffer into the other, and BOTH come back: out with the sums (its words behind the
 * n-th of every array as the caller left them), in as the device holds it behind the scan (unchanged, if the scan is right).  Needs
 * a created handle, nothing uploaded. */
int ig_debug_scan64(ig_ctx* ctx, uint64_t* in, int32_t n, int32_t n_arrays, int64_t stride, uint64_t* out);
/* tests: the row builder of the reports (the counting sort into rows, the sort of every row in one of three forms and, reduce != 0,
 * the sum of the runs of equal columns) over caller data, unchanged: entry k goes to row lo[k] (negative: no entry) as the word
 * word[k] = column << 32 | count.  combine: as ig_debug_assembly_contacts_combine, of this call; the limits of
 * ig_debug_assembly_contacts_limits hold.  *n_entries: the entries with a row; *n_out: the entries of the result (behind a reduction
 * the distinct (row, column)); forms: as ig_debug_assembly_contacts_forms.  The result waits on the host for ig_debug_rows_fetch;
 * nothing stays on the device.  Refused: negative n or n_rows, lo[k] >= n_rows, a column of 2^31 or more.  Needs a created handle,
 * nothing uploaded: the sub-fragment table, the contacts and the state are not read. */
int ig_debug_rows_build(ig_ctx* ctx, const int32_t* lo, const uint64_t* word, int64_t n, int32_t n_rows, int32_t reduce, int32_t combine,
                        int64_t* n_entries, int64_t* n_out, int64_t forms[8]);
/* the last ig_debug_rows_build's result: rowptr[n_rows + 1] (n_rowptr: the caller's capacity) and its n_out entries (capacity: the
 * caller's) -- not reduced: word[n_out], sorted inside every row as unsigned 64-bit words (col and count are not written); reduced:
 * col[n_out] and count[n_out] (word is not written) */
int ig_debug_rows_fetch(ig_ctx* ctx, int64_t* rowptr, int64_t n_rowptr, uint64_t* word, int32_t* col, int64_t* count, int64_t capacity);
/* tests: the combining idiom of the passes over the contacts (a run of a wave's lanes with an equal destination is summed inside the
 * wave and issues one atomic) over caller data, unchanged: entry k adds values[k] to out[keys[k]] (a negative key: no entry), n
 * entries in order, 64 to a wave, 256 to a workgroup.  wide: 0 the sums inside the wave are made in 32 bits (no run may overflow
 * them), else in 64.  out[n_dest]: the sums; *atomics: the atomics issued -- one per run with a key whose values do not sum to 0.
 * Refused: a NULL pointer, negative n or n_dest, keys[k] >= n_dest.  Needs a created handle, nothing uploaded. */
int ig_debug_wave_runs(ig_ctx* ctx, const int32_t* keys, const int64_t* values, int64_t n, int32_t n_dest, int32_t wide, int64_t* out, int64_t* atomics);
/* join support: the form of the two passes over the contacts of THIS handle's builds: 1 a run of a wave's lanes with the same row
 * issues one atomic per emission, 0 one atomic per emission (the yardstick), negative: the form the library ships.  The result is
 * the same.  The limits of ig_debug_assembly_contacts_limits hold for this feature's sorts too. */
int ig_debug_join_support_combine(ig_ctx* ctx, int32_t combine);
/* the last join support build's work lists, as ig_debug_assembly_contacts_forms */
int ig_debug_join_support_forms(ig_ctx* ctx, int64_t out8[8]);
/* the build n times (with the model pass if parameters are set), hipEvents around each pass: ms_n[n][9] = {ends, count, scan,
 * scatter, sort short, sort lds, sort long, reduce, model}; the last result stays built; *checksum (may be NULL): its rows, columns
 * and observed, each word weighted by its place */
int ig_debug_join_support_time(ig_ctx* ctx, int32_t window, int32_t n, float* ms_n, int64_t* checksum);
/* the expected map: the form of THIS handle's builds: 0 the form the library ships, 1 rows (one thread per position, atomics: the
 * yardstick), 2 tiles (one workgroup per pixel pair that can hold a cis pair, no atomics on the images), 3 tiles without the
 * constant-tile shortcut.  With one position per pixel the row form runs whatever is set.  The images are the same. */
int ig_debug_expected_map_form(ig_ctx* ctx, int32_t form);
/* the build under that form (as above) n times, hipEvents around each (zero, the passes, the mirrors; the tile form's wait for the
 * size of its list included): ms_n[n]; *checksum (may be NULL): the three images of the last build, the two pair counts and max_q,
 * each word weighted by its place: every form must agree on it */
int ig_debug_expected_map_time(ig_ctx* ctx, int32_t max_side, int32_t form, int32_t n, float* ms_n, int64_t* checksum);
/* placement support: the form of the scan of THIS handle's calls: 0 the form the library ships (a wave per row of more than
 * PLACE_WAVE_ENTRIES summed entries, a thread per shorter row), 1 a thread per row (the yardstick), 2 a wave per row.  The arrays are
 * the same.  The limits of ig_debug_assembly_contacts_limits hold for this feature's sorts too. */
int ig_debug_placement_support_form(ig_ctx* ctx, int32_t form);
/* the last placement support call's work lists, as ig_debug_assembly_contacts_forms */
int ig_debug_placement_support_forms(ig_ctx* ctx, int64_t out8[8]);
/* the call n times, hipEvents around each pass: ms_n[n][10] = {records, count, rows, scatter, sort short, sort lds, sort long, reduce,
 * prefix, scan}; *checksum (may be NULL): the arrays of the last call, each word weighted by its place: every form must agree on it */
int ig_debug_placement_support_time(ig_ctx* ctx, int32_t window, int32_t min_hosts, int32_t n, float* ms_n, int64_t* checksum);
/* orientation support: one pass n times, hipEvents around each (zero + kernel): ms_n[n].  pass 0, the observed pass -- form 0: one
 * atomic per counted end (the yardstick), 1: equal row ends summed inside the wave first; pass 1, the model pass -- form 0: as
 * shipped (a wave per segment of up to ORIENT_WAVE_PAIRS terms, a workgroup beyond), 1: a wave per segment, 2: a workgroup per
 * judged segment.  *checksum (may be NULL): the words the last pass wrote (pass 0: the quadrants and the seven scalars; pass 1:
 * expected_q), each weighted by its place: every form of a pass must agree on it */
int ig_debug_orientation_support_time(ig_ctx* ctx, int32_t window, int32_t n_seg, const int32_t* seg_first, const int32_t* seg_last, int32_t pass,
                                      int32_t form, int32_t n, float* ms_n, int64_t* checksum);

/* ---- balancing the contact map of the current genome: one weight per unit by iterative correction (the rule:
 * instagraal_amd/balance.py).  The device reproduces the rule's arrays byte for byte. */
/* The rows.  level: 0 the positions of the genome order, 1 the placed bins along it, 2 the pixels of ig_contact_map under max_side
 * (read at level 2 only).  Every contact with both ends placed in units u != v, |u - v| >= ignore_diags (>= 1), gives the entries
 * (u, v, c) and (v, u, c); rows sorted by column, equal columns summed.  scalars[8] = {unplaced_observed, within_observed,
 * band_observed, kept_observed, entries, n_placed, n_units, entries_out}.  Needs all contacts on this handle and no chain or
 * nuisance step in flight; refuses a unit whose counts sum to 2^53 or more.  The rows stay on the device until ig_balance_release
 * (or the next build). */
int ig_balance_build(ig_ctx* ctx, int32_t level, int32_t max_side, int32_t ignore_diags, int64_t* n_units, int64_t* n_entries, int64_t scalars[8]);
/* rowptr[n_units + 1] (capacity: its words), and per unit its entries and the sum of their counts */
int ig_balance_rows(ig_ctx* ctx, int64_t* rowptr, int64_t* nnz, int64_t* total, int64_t capacity);
/* entries first .. first + n - 1 of the built rows */
int ig_balance_fetch(ig_ctx* ctx, int64_t first, int64_t n, int32_t* col, int64_t* count);
/* The iterations of the rule over the built rows from b0[n_units] (the caller's mask: 0.0 where a unit is masked): stops after the
 * first iteration with variance < tol (tol = 0: never) or after max_iters.  b, marg_final: [n_units] (marg_final from the final b);
 * variance[max_iters]: one word per iteration done, zero beyond; *converged: 1 / 0.  No unit-sized array crosses to the host inside
 * the loop.  With no entry, or b0 zero everywhere, *n_iters = 0 and nothing is launched. */
int ig_balance_run(ig_ctx* ctx, const double* b0, double tol, int32_t max_iters, double* b, double* marg_final, double* variance, int32_t* n_iters,
                   int32_t* converged);
int ig_balance_release(ig_ctx* ctx);
/* the form of k_bal_marginals of THIS handle: 0 the form the library ships, 1 a wave per row (the yardstick), 2 packed (four rows of at
 * most 16 entries share a wave).  The bytes are the same. */
int ig_debug_balance_form(ig_ctx* ctx, int32_t form);
/* the iterations ig_balance_run enqueues between two looks at the device's done flag (0: the default).  The results are the same. */
int ig_debug_balance_group(ig_ctx* ctx, int32_t group);
/* the ordered sum (balance.lane_sum) of every row of caller data in the handle's form: values[rowptr[n_rows]], rowptr[n_rows + 1]
 * from 0 and non-decreasing, out[n_rows].  A created handle is enough. */
int ig_debug_lane_sums(ig_ctx* ctx, const double* values, const int64_t* rowptr, int64_t n_rows, double* out);
/* over the built rows, from b = 1 and in the handle's form, n times with hipEvents around each: what = 0 k_bal_marginals alone, 1 one
 * whole iteration (marginals, mean, update, variance): ms_n[n] */
int ig_debug_balance_time(ig_ctx* ctx, int32_t what, int32_t n, float* ms_n);
/* the build n times, hipEvents around each pass: ms_n[n][8] = {units, count, rows, scatter, sort short, sort lds, sort long, reduce};
 * the last build's rows stay */
int ig_debug_balance_build_time(ig_ctx* ctx, int32_t level, int32_t max_side, int32_t ignore_diags, int32_t n, float* ms_n);

/* ---- gap support: the distance the contacts put across each join of the current genome (the rule: instagraal_amd/gap_support.py;
 * DESIGN.md 4.20).  The device reproduces the rule's arrays byte for byte. */
/* junction[n_junc] (n_junc >= 1): positions 1 .. T - 1 of the genome order, strictly ascending, each between two positions of one
 * placed contig; anything else is an error of the whole call.  gaps_kb[n_gaps], 2 <= n_gaps <= 64: finite, strictly ascending,
 * gaps_kb[0] == 0.  window: 1 .. 256 positions.  Per junction: status (0 judged, 2 on a ring: its row is 0), geometry (the canonical
 * id of the contig, left, right, 0), observed, pairs, and per junction and gap k, in units of 2^-32, log_q = the sum over the
 * contacts that span the junction inside the window of count * ig_quantize of ig_log10 of E_k and expected_q = the sum over the pairs
 * that could of ig_quantize of E_k, E_k = ig_rippe at separation + gaps_kb[k] under parameter set 0 (model == 0: expected_q is not
 * computed and may be NULL).  scalars[8] = {unplaced, trans, ring, counted, uncounted, contributions, n_judged, n_placed}.  On a
 * sharded handle observed, log_q and the first six scalars add up over the ranks; pairs and expected_q are whole on every rank.
 * Needs the contacts, a state and parameters, no chain or nuisance step in flight.  Refuses, with nothing written to the caller's
 * arrays and the handle usable: a malformed list or grid, "model value too large for this window" (the largest |value| times
 * w (w + 1) / 2 reaches 2^62) and "too many contacts across one junction for this model" (the largest |log| times the largest
 * observed reaches 2^62).  Writes nothing a move reads; its buffers are kept from call to call and freed by ig_destroy. */
int ig_gap_support(ig_ctx* ctx, int32_t window, int32_t model, int32_t n_junc, const int32_t* junction, int32_t n_gaps, const float* gaps_kb, int32_t* status,
                   int32_t* geometry /* [4 n_junc] */, int64_t* observed, int64_t* pairs, int64_t* log_q /* [n_junc * n_gaps] */,
                   int64_t* expected_q /* [n_junc * n_gaps], NULL iff !model */, int64_t scalars[8]);
/* the two model values of n separations on the CPU, from include/ig_detmath.h: e_q = ig_quantize of ig_rippe at s under params, l_q =
 * ig_quantize of ig_log10 of that value; params: the eight floats of ig_params in its order.  No context, no GPU: HIP is not initialised. */
int ig_model_values_host(const float params[8], const float* s, int64_t n, int64_t* e_q, int64_t* l_q);
/* one pass of the gap support n times, hipEvents around each (zero + kernel): ms_n[n].  pass 0: the observed pass (one atomic per
 * word); 1: the model pass as shipped (a wave per junction of up to GAP_WAVE_TERMS terms, a workgroup beyond), 2: a wave per junction,
 * 3: a workgroup per judged junction.  *checksum (may be NULL): the words the last pass wrote (pass 0: observed, log_q and the six
 * scalars; else expected_q), each weighted by its place: every form of the model pass must agree on it */
int ig_debug_gap_support_time(ig_ctx* ctx, int32_t window, int32_t n_junc, const int32_t* junction, int32_t n_gaps, const float* gaps_kb, int32_t pass, int32_t n,
                              float* ms_n, int64_t* checksum);

/* ---- fixed-resolution maps of the current genome: the contacts at a caller's unit per position, and a built level coarsened to
 * the next (the rule: instagraal_amd/zoom_levels.py).  The device reproduces the rule's arrays byte for byte. */
/* ig_assembly_contacts_build at level 1 with the caller's units: unit[n_positions] is the unit of every position of
 * ig_contact_map_order, non-decreasing along the order, inside 0 .. n_units - 1; it may step by more than one (the rows of the
 * units without a position are empty).  Refused on the host before any work on the device: n_units of 2^31 or more, a table that is
 * not monotone or out of range; then n_positions != T.  The result is a snapshot as ig_assembly_contacts_build's (n_units rows):
 * ig_assembly_contacts_rows, _fetch and _release serve it, the same scalars, the same guards, sharding as there.  The earlier
 * snapshot is gone whatever happens. */
int ig_assembly_contacts_build_units(ig_ctx* ctx, const int32_t* unit, int64_t n_positions, int64_t n_units, int64_t* n_entries, int64_t scalars[8]);
/* Replaces the built, summed snapshot (ig_assembly_contacts_build at level 1, _build_units, or an earlier coarsening) by its
 * coarsening: entry (lo, hi, c) goes to (coarse_of_unit[lo], coarse_of_unit[hi]), equal entries are summed in 64 bits (a count may
 * exceed 2^32).  coarse_of_unit[n_units]: non-decreasing, inside 0 .. n_coarse - 1; n_units: the snapshot's.  The contacts are not
 * read again.  scalars: {0, 1 the entries read, 2 contacts_kept, 3, 4, 5 as the snapshot's build gave them, 6 n_coarse, 7
 * entries_out = *n_entries}.  Refused, with NOTHING left built: no snapshot, a level 0 snapshot, another n_units, a map that is not
 * monotone or out of range, a coarse row of 2^32 entries or more before summing.  Device memory during the call: the old and the
 * new level, 8 bytes per old entry (16 with long rows), a bit per entry.  On a sharded handle the coarsening of the shard's snapshot
 * is that shard of the coarsened whole.  Writes nothing a move reads. */
int ig_assembly_contacts_coarsen(ig_ctx* ctx, const int32_t* coarse_of_unit, int64_t n_units, int64_t n_coarse, int64_t* n_entries, int64_t scalars[8]);
/* ig_balance_build at level 1 with the caller's units (the table as for ig_assembly_contacts_build_units, the same refusals);
 * ig_balance_rows, _fetch, _run and _release then work on it unchanged. */
int ig_balance_build_units(ig_ctx* ctx, const int32_t* unit, int64_t n_positions, int64_t n_units, int32_t ignore_diags, int64_t* n_entries, int64_t scalars[8]);
/* tests: the coarsening over caller data, unchanged: the CSR level rowptr[n_rows + 1] (from 0, non-decreasing), col and count
 * [rowptr[n_rows]] (columns inside 0 .. n_rows - 1) under coarse_of_unit[n_rows] into n_coarse rows; the limits of
 * ig_debug_assembly_contacts_limits hold; forms: as ig_debug_assembly_contacts_forms, of the segments.  The result waits on the host
 * for ig_debug_zoom_fetch; nothing stays on the device.  Needs a created handle, nothing uploaded. */
int ig_debug_zoom_coarsen(ig_ctx* ctx, const int64_t* rowptr, const int32_t* col, const int64_t* count, int64_t n_rows, const int32_t* coarse_of_unit,
                          int64_t n_coarse, int64_t* n_out, int64_t forms[8]);
/* the last ig_debug_zoom_coarsen's result: rowptr[n_coarse + 1] (n_rowptr: the caller's capacity), col and count [n_out] (capacity) */
int ig_debug_zoom_fetch(ig_ctx* ctx, int64_t* rowptr, int64_t n_rowptr, int32_t* col, int64_t* count, int64_t capacity);
/* the coarsening of the built snapshot under coarse_of_unit (NULL: two units to one, n_units and n_coarse are not read) n times, hipEvents
 * around each pass: ms_n[n][6] = {segment starts, words, sort short, sort lds, sort long, reduce}.  The snapshot is read only and stays
 * as it is; *checksum (may be NULL): the rows, columns and counts of the last repeat, each word weighted by its place */
int ig_debug_zoom_time(ig_ctx* ctx, const int32_t* coarse_of_unit, int64_t n_units, int64_t n_coarse, int32_t n, float* ms_n, int64_t* checksum);

/* ---- segment placement support: where the contacts say a run of bins belongs, and which way round (the rule:
 * instagraal_amd/segment_placement.py).  The guests are the n_seg segments [seg_first[i], seg_last[i]] of positions of
 * the genome order (ascending, disjoint, each inside one placed contig; they need not cover the order); each gets what
 * ig_placement_support gives a bin -- home, the best site, the runner-up, the segment itself taken out of the order -- and at each of
 * the three sites the four sums HL, HR, TL, TR of its contacts by the arm of the segment they touch (head, tail: its outermost
 * min(n / 2, window) positions) and the part of the site's window the other end lies in (left, right).  The device reproduces the
 * rule's arrays byte for byte, whatever the form of the scan (ig_debug_placement_support_form holds here too: it is the same kernel).
 * ints: 12 arrays of n_seg int32 -- status (0 guest, 2 on a ring), contig, offset, n_positions, home_hosts, best_contig, best_offset,
 * best_hosts, second_contig, second_offset, second_hosts, arm --; longs: 6 arrays of n_seg int64 -- home_left, home_right, best_left,
 * best_right, second_left, second_right --; quadrants: [n_seg][3][4], the sites home, best, second; scalars: unplaced_observed,
 * ring_observed, within_segment_observed, counted_observed, uncounted_observed, entries, n_contigs, n_guests, n_placed.  The arrays may
 * be NULL with n_seg == 0.  A call that fails leaves the outputs untouched and the handle usable; nothing stays on the device.  Needs the
 * sub-fragment table, the contacts and a state, all contacts on one handle, and no nuisance step or chain in flight. */
int ig_segment_placement(ig_ctx* ctx, int32_t window, int32_t min_hosts, int32_t n_seg, const int32_t* seg_first, const int32_t* seg_last, int32_t* ints,
                         int64_t* longs, int64_t* quadrants, int64_t scalars[9]);
/* the call n times with hipEvents around each pass: ms_n[n][11] = {records, count, rows, scatter, sort short, sort lds, sort long, reduce,
 * prefix, scan, quadrants}; *checksum (may be NULL): every output word of the last call -- ints, longs, quadrants, scalars -- weighted by
 * its place */
int ig_debug_segment_placement_time(ig_ctx* ctx, int32_t window, int32_t min_hosts, int32_t n_seg, const int32_t* seg_first, const int32_t* seg_last, int32_t n,
                                    float* ms_n, int64_t* checksum);

/* ---- segment edits: the moves the block-level reports propose, scored exactly and applied (the rule: instagraal_amd/rearrange.py;
 * DESIGN.md 4.23).  An edit is five int32: first_bin, last_bin, anchor, side, flip -- the bins of one linear contig from first_bin to
 * last_bin (in the current order) are taken out, reversed with their ori negated if flip, and put back where they were (anchor -2),
 * made a contig of their own (anchor -1) or inserted directly behind (side 0) or in front of (side 1) the bin anchor, a bin outside
 * the segment in a linear contig.  status: 0 ok, 1 a bin out of range, 2 the two bins not in one contig or in the wrong order, 3 a
 * ring, 4 the anchor inside the segment, 5 anchor, side or flip out of range.  The device reproduces the rule's states byte for byte.
 * All three calls need the sub-fragment table, the contacts, a state and the parameters, all contacts on one handle, and no nuisance
 * step or chain in flight. */
/* The five exact sums of the genome every edit of edits[n_edits][5] would leave, limbs[n_edits][5] in the order of
 * ig_full_likelihood's limbs5, with nz[n_edits] and z[n_edits] formed as that call forms them; an edit that is refused (status != 0)
 * gets the sums of the current genome.  form 0 (the delta form): the maintained sums plus one pass over the contacts and one over the
 * sub-fragments per chunk of up to 64 edits, terms evaluated only where a contig an edit touches is involved; form 1 (the whole form,
 * the definition): the from-scratch passes on the tables of every edited genome.  Both give the same limbs.  Any n_edits: the list is
 * worked off in chunks of 64 or fewer, as many as the free device memory holds (per edit: 44 N + 20 M bytes); when one edit does not
 * fit the call fails before it allocates and names the bytes it needs.  Reads the current state and changes nothing a move reads.  The
 * buffers are kept from call to call and freed by ig_destroy. */
int ig_edit_score(ig_ctx* ctx, int32_t n_edits, const int32_t* edits, int32_t form, int32_t* status, int64_t* limbs, double* nz, double* z);
/* tests: the state one edit would leave, soa17 in the order of ig_upload_state with the INTERNAL contig ids (a new contig: the next
 * free id); nothing is committed.  A refused edit returns the current state. */
int ig_edit_state(ig_ctx* ctx, const int32_t edit[5], int32_t* soa17, int32_t* status);
/* Commits one edit: its dynamic arrays become the live state, a new contig uses up the next free id, the stale insert flags are
 * cleared as ig_upload_state clears them, the moves scored ahead are dropped, and everything a move reads is rebuilt from the state
 * (tables, maintained sums, genome distance).  The initial genome, the blacklist and the parameters stay.  limbs5 (may be NULL): the
 * maintained sums behind the call.  A status other than 0 leaves everything as it was. */
int ig_edit_apply(ig_ctx* ctx, const int32_t edit[5], int32_t* status, int64_t* limbs5);
/* ig_edit_score n times with hipEvents around each pass, summed over the chunks: ms_n[n][6] = {plan, state, tables, delta, zero,
 * whole} (the passes of the other form stay 0); *checksum (may be NULL): the statuses, then the limbs of the last call, each word
 * weighted by its place: the two forms agree on it */
int ig_debug_edit_time(ig_ctx* ctx, int32_t n_edits, const int32_t* edits, int32_t form, int32_t n, float* ms_n, int64_t* checksum);

/* ---- cut and join scores: the closed part of the likelihood change of EVERY cut of a linear contig and of EVERY link of two linear
 * contigs, as exact integers in the units of ig_edit_score, from one pass over the contacts each (the rule, stated once:
 * instagraal_amd/cut_join.py).  A cut in front of bin f (f in a linear contig, prev[f] >= 0) is the edit
 * (f, last bin of the contig, NEW_CONTIG, 0, 0); a link (sa, sb) of the linear contigs a < b (numbered 0 .. K - 1 in ascending
 * internal contig id; side 0: the head, 1: the tail) keeps a and moves all of b behind a's last bin (sa = 1, flipped where sb = 1) or
 * in front of a's first bin (sa = 0, flipped where sb = 0).  Delta limbs are differences of limbs {nz hi, nz lo, z hi, z lo, intra
 * pairs}, hi = q >> 32 and lo = (uint32) q summed apart, not normalised; a delta is (nz + z) of the maintained sums plus the delta
 * limbs minus (nz + z) of the maintained sums, each formed as ig_full_likelihood forms them.  What is left out is the internal
 * part: the contacts whose two ends stay in one contig on one side, whose f32 separation changes only by rounding (and by the mirrored
 * reference points of a flipped contig); ig_edit_score has it.  All calls need the sub-fragment table, the contacts, a state and the
 * parameters, all contacts on one handle, no nuisance step or chain in flight; they change nothing a move reads; their buffers are
 * kept from call to call (those sized by the contigs and the pairs grow only; a state of another size frees them all and starts again)
 * and are freed by ig_destroy. */
/* per bin f: valid[N] (a cut exists), contacts[N] (stored contacts that span the junction), limbs[N][5], delta[N]; 0 where no cut exists */
int ig_cut_scores(ig_ctx* ctx, int32_t* valid, int64_t* contacts, int64_t* limbs, double* delta);
/* every pair a < b of linear contigs with a contact between them: the build leaves the result on the host side of the handle until
 * the next build or ig_join_scores_release.  fetch: per contig head_bin, tail_bin, n_sub, length_bp [K]; CSR rowptr[K + 1], col (b,
 * ascending); per pair contacts, nz[4][2] (link 2 sa + sb), z[2] (equal for the four links), dni, delta[4]. */
int ig_join_scores_build(ig_ctx* ctx, int64_t* n_contigs, int64_t* n_pairs);
int ig_join_scores_fetch(ig_ctx* ctx, int32_t* head_bin, int32_t* tail_bin, int32_t* n_sub, int32_t* length_bp, int64_t* rowptr, int32_t* col, int64_t* contacts,
                         int64_t* nz, int64_t* z, int64_t* dni, double* delta);
int ig_join_scores_release(ig_ctx* ctx);
/* tests: the form of the join pass, -1: by the number of pairs (up to 256: accumulators in LDS, beyond: global atomics per run of a
 * wave), 0: LDS (windows of 256 pairs, one launch each), 1: atomics per run.  Both give the same bytes. */
int ig_debug_cut_join_form(ig_ctx* ctx, int32_t form);
/* the LIFT_C_* words of the pairs' rows of the last finished build (kept behind ig_join_scores_release) */
int ig_debug_join_scores_forms(ig_ctx* ctx, int64_t out8[8]);
/* what = 0: ig_cut_scores, 1: ig_join_scores_build, n times with hipEvents around each pass: ms_n[n][12] = {span, scan, zero, count,
 * rowscan, scatter, sort_short, sort_lds, sort_long, reduce, terms, join_zero} (the other report's passes stay 0); *checksum (may be
 * NULL): the integer words of the last result, each weighted by its place: the forms agree on it */
int ig_debug_cut_join_time(ig_ctx* ctx, int32_t what, int32_t n, float* ms_n, int64_t* checksum);
/* eval_q's ring-free branch on the CPU from include/ig_detmath.h, hot path selection included: q[k] = the quantised term of a contact
 * of count[k] at separation s[k] kb and rank distance d[k] (trans[k] != 0: a trans pair; s and d play no part).  No context, no GPU. */
int ig_contact_terms_host(const float params[8], float mean_kb, const float* s, const int32_t* d, const int32_t* trans, const int32_t* count, int64_t n, int64_t* q);
/* tests: eval_q itself on the device for the same inputs (s >= 0, 0 <= d < 2^28), under parameter set 0 and its P_z table: the two agree
 * bit for bit */
int ig_debug_contact_terms(ig_ctx* ctx, const float* s, const int32_t* d, const int32_t* trans, const int32_t* count, int64_t n, int64_t* q);
/* zero_q of a linear contig on the CPU: the sub-fragment of rank pos[k] in a contig of len[k] sub-fragments.  No context, no GPU. */
int ig_zero_terms_host(const float params[8], float mean_kb, const int32_t* pos, const int32_t* len, int64_t n, int64_t* q);

/* ---- read pairs lifted onto the current genome: Hi-C read pairs, aligned to the INPUT contigs, in the coordinates of the scaffolds as
 * they stand, kept on the device; from them the pixels at any unit and the distance histogram per strand combination (the rule, stated
 * once: instagraal_amd/pairs_lift.py).  A SESSION lives between ig_pairs_begin and ig_pairs_end (ig_destroy frees a
 * live one).  It is begun under one genome: every later call compares the state with the one the session was begun under and refuses
 * once a move, an edit or an upload has changed it (end the session and begin again with a table of the new genome).  All calls need a
 * state, the whole genome on one handle, no nuisance step or chain in flight; they change nothing a move reads.
 *
 * The source table: n_intervals intervals sorted by (contig, src_start), src_rowptr[n_contigs + 1] over the contig ids; per interval
 * [src_start, src_end) on its contig (0-based, half-open, not overlapping), the rank of its scaffold among the n_scaffolds placed ones
 * (at most 2^30 of them; -1: not placed), new_start inside the scaffold, reversed (0 / 1) and its position in the genome order (0 .. n_positions - 1);
 * scaffold_len[n_scaffolds] in bp, each at most 2^31 - 1; bin_unit[n_positions]: the unit of every position among the n_bin_units placed
 * bins.  reserve_pairs: room in the store from the start (it grows by itself, under a check of the free device memory: a refusal
 * leaves the session as it was). */
int ig_pairs_begin(ig_ctx* ctx, const int32_t* src_rowptr, int32_t n_contigs, const int32_t* src_start, const int32_t* src_end, const int32_t* new_start,
                   const int32_t* scaffold, const uint8_t* reversed, const int32_t* position, int64_t n_intervals, const int64_t* scaffold_len, int32_t n_scaffolds,
                   const int32_t* bin_unit, int64_t n_positions, int64_t n_bin_units, int64_t reserve_pairs);
/* One chunk of n pairs: contig ids (anything outside 0 .. n_contigs - 1: unknown) and 1-based positions of the two ends; strands (may
 * be NULL: all '+'): bit 0 set where end 1 was read on '-', bit 1 where end 2 was.  The nine per-pair outputs (all given, or all NULL)
 * are in input order: scaffold (-1), 1-based position (0), position of the interval in the genome order (-1) and reversed bit per end;
 * status 0 kept, 1 end 1 not covered, 2 end 2 not covered, 3 an end on an unplaced sub-fragment.  The kept pairs are appended to the
 * store (in no particular order).  scalars: {pairs in, kept, end 1 not covered, end 2 not covered, unplaced, pairs stored, 0, 0}. */
int ig_pairs_lift(ig_ctx* ctx, const int32_t* c1, const int32_t* p1, const int32_t* c2, const int32_t* p2, const uint8_t* strands, int64_t n, int32_t* scaffold1,
                  int32_t* pos1, int32_t* unit1, uint8_t* rev1, int32_t* scaffold2, int32_t* pos2, int32_t* unit2, uint8_t* rev2, uint8_t* status, int64_t scalars[8]);
/* The pixels of the stored pairs: kind 0 the positions, 1 the placed bins, 2 fixed bins of binsize bp (first_unit[scaffold] + position
 * / binsize), 3 the scaffolds; keys (min, max), equal keys summed, the diagonal kept.  The result REPLACES the handle's
 * assembly-contacts snapshot: ig_assembly_contacts_rows, _fetch, _coarsen and _release serve it as they serve a build from the
 * contacts.  scalars: the eight words of ig_assembly_contacts_build (entries: the stored pairs). */
int ig_pairs_pixels_build(ig_ctx* ctx, int32_t kind, int64_t binsize, int64_t* n_units, int64_t* n_entries, int64_t scalars[8]);
/* The stored pairs with both ends on one scaffold by distance and strand combination: counts[4][n_edges - 1] (++, +-, -+, --), bin =
 * clip(the last edge <= |pos2 - pos1|, 0, n_edges - 2); 2 <= n_edges <= 512 edges in bp, >= 0, ascending.  flip_strands: an end on a
 * reversed interval has its strand flipped.  scalars: {pairs stored, counted, on two scaffolds, 0 ...}. */
int ig_pairs_law(ig_ctx* ctx, const int64_t* edges_bp, int32_t n_edges, int32_t flip_strands, int64_t* counts, int64_t scalars[8]);
/* empties the store; the table and the buffers stay */
int ig_pairs_clear(ig_ctx* ctx);
int ig_pairs_end(ig_ctx* ctx);
/* the three passes n times with hipEvents around each: every repeat empties the store, lifts the chunk, counts the law and builds the
 * pixels: ms_n[n][9] = {lift, count, scan, scatter, sort_short, sort_lds, sort_long, reduce, law}; *checksum (may be NULL): the scalars
 * and the histogram of the last repeat, each word weighted by its place */
int ig_debug_pairs_time(ig_ctx* ctx, const int32_t* c1, const int32_t* p1, const int32_t* c2, const int32_t* p2, const uint8_t* strands, int64_t n_pairs, int32_t kind,
                        int64_t binsize, const int64_t* edges_bp, int32_t n_edges, int32_t n, float* ms_n, int64_t* checksum);

/* ---- the input folder from an assembly FASTA and read pairs: the restriction digest of the records, G + C per fragment, the fragment
 * of every pair end and the pixels (the rule, stated once: instagraal_amd/pre.py).  A SESSION lives between
 * ig_pre_begin and ig_pre_end (ig_destroy frees a live one) on a created handle; it needs no contacts and no state and changes nothing
 * a move reads; no nuisance step or chain may be in flight.
 *
 * seq: n_bytes bytes, the records one behind the other with a zero byte (the separator) behind each: rec_off[0] == 0, rec_off[r + 1]
 * == rec_off[r] + rec_len[r] + 1, n_bytes == rec_off[n_records - 1] + rec_len[n_records - 1] + 1.  The offsets are 64-bit (a genome
 * may exceed 2^31 bytes), a record is 1 .. 2^31 - 2 bases of ABCDGHKMNRSTVWY in either case; anything else is refused naming the record
 * and the position.  The bytes go to the device in pieces. */
int ig_pre_begin(ig_ctx* ctx, const uint8_t* seq, int64_t n_bytes, const int64_t* rec_off, const int32_t* rec_len, int32_t n_records);
/* The digest under 1 .. 4 enzymes: site_len[e] (1 .. 16) letters, the cut behind cut[e] (0 .. site_len[e]) of them, masks[e][16]: per
 * site letter the bits of the bases it accepts (A 1, C 2, G 4, T 8), or 16: any letter (the site letter N).  A match at the 0-based
 * start s of a record cuts at s + cut; the cuts of all enzymes with 0 and the record's length bound its fragments.
 * frags_per_record[n_records], *n_frags: their numbers.  ms (may be NULL): the times of the four passes {sites, scan, cuts, fragments}.
 * An earlier digest of the session, its store and its pixels are gone. */
int ig_pre_digest(ig_ctx* ctx, int32_t n_enzymes, const int32_t* site_len, const int32_t* cut, const uint8_t* masks, int64_t* frags_per_record, int64_t* n_frags,
                  float* ms);
/* the fragments first .. first + n - 1 in the order of the records: record, start, end (0-based, half-open, inside the record), G + C */
int ig_pre_fragments(ig_ctx* ctx, int64_t first, int64_t n, int32_t* frag_rec, int32_t* start, int32_t* end, int32_t* gc_count);
/* One chunk of pairs: the record (-1: unknown) and the 1-based position of both ends.  The fragment of an end is the last of its
 * record that starts at or before position - 1: none for a position <= 0 or an unknown record, the record's last for a position beyond
 * its end.  A pair with both is appended to the session's store, which grows.  scalars: the chunk's {pairs_in, pairs_kept,
 * end1_without_fragment, end2_without_fragment, ends_beyond_record}, the pairs stored in all, 0, 0.  ms (may be NULL): the kernel's
 * time.  An earlier build's pixels are gone. */
int ig_pre_add_pairs(ig_ctx* ctx, const int32_t* c1, const int32_t* p1, const int32_t* c2, const int32_t* p2, int64_t n, int64_t scalars[8], float* ms);
/* The pixels of the store: every stored pair adds 1 at (min, max) of its two fragments; rows by bin1, columns ascending, equal ones
 * summed.  scalars: {pairs_in, pairs_kept, end1_without_fragment, end2_without_fragment, ends_beyond_record, pixels} over every chunk
 * since the digest or ig_pre_clear, the fragments, the stored pairs.  ms (may be NULL): the seven passes of the row builder. */
int ig_pre_pixels_build(ig_ctx* ctx, int64_t* n_pixels, int64_t scalars[8], float* ms);
/* rowptr[n_frags + 1] of the built pixels (n_rowptr: the caller's capacity) */
int ig_pre_pixels_rows(ig_ctx* ctx, int64_t* rowptr, int64_t n_rowptr);
/* the pixels first .. first + n - 1 in the order of (bin1, bin2): bin2 and the count */
int ig_pre_pixels_fetch(ig_ctx* ctx, int64_t first, int64_t n, int32_t* col, int64_t* count);
/* empties the store and its scalars and drops the pixels; the sequence, the digest and the buffers stay */
int ig_pre_clear(ig_ctx* ctx);
int ig_pre_end(ig_ctx* ctx);

/* ---- 4DN pairs text on the device: the lines of a chunk of bytes, their fields, the two decimal positions, the strand bits and the
 * contig names (the rule, stated once: instagraal_amd/pairs_text.py).  A SESSION lives between ig_text_begin and
 * ig_text_end (ig_destroy frees a live one) on a created handle; it needs no contacts and no state and changes nothing a move reads; no
 * nuisance step or chain may be in flight.  ig_text_begin while a session is live is refused; ig_text_end without one does nothing.
 *
 * The vocabulary: name k is name_bytes[name_off[k] .. name_off[k + 1]) and has the id name_id[k]; where a name stands twice the later
 * id wins.  A field is looked up by its exact bytes (64-bit FNV-1a into an open-addressing table at load <= 0.5, a hit confirmed by the
 * bytes); an unknown name, the empty one included, is -1. */
int ig_text_begin(ig_ctx* ctx, const uint8_t* name_bytes, const int64_t* name_off, const int32_t* name_id, int32_t n_names);
/* One chunk of whole lines, 0 <= n_bytes <= 2^30 (refused on the argument beyond that): every line ends in '\n' except possibly the
 * last; line j starts behind the j-th '\n'.  cols: the column indices of chr1, pos1, chr2, pos2, strand1, strand2 (0 .. 65535).  A
 * line's status: 1 COMMENT (its first byte is '#'), 2 MALFORMED (fewer than max(cols[0..3]) + 1 fields, split at '\t' only), 3 DEFERRED
 * (a position that is not exactly [+-]?[0-9]{1,18}: left to the caller), 0 DATA.  The lines from the first one that starts with
 * "#columns:" on are not parsed (status COMMENT, counted nowhere but in `lines`).  A chunk that holds a '\r' or a byte >= 0x80 is not
 * parsed at all: to_host is raised, nothing else of the result is defined and the call succeeds.
 * scalars: {lines, data, comment, malformed, deferred, first_columns_line (-1: none), to_host, 0}.  ms (may be NULL): the times of the
 * four passes {mark, scan, parse, compact}. */
int ig_text_parse(ig_ctx* ctx, const uint8_t* bytes, int64_t n_bytes, const int32_t cols[6], int64_t scalars[8], float* ms);
/* the last chunk's result: status [lines], line_start [lines + 1], contig id and position of both ends and the strand code (bit 0: end
 * 1 on '-', bit 1: end 2) of the DATA lines in input order [data], the indices of the DEFERRED lines [deferred]; any pointer may be NULL */
int ig_text_fetch(ig_ctx* ctx, uint8_t* status, int32_t* line_start, int32_t* c1, int64_t* p1, int32_t* c2, int64_t* p2, uint8_t* strands, int32_t* deferred);
/* The DATA pairs of the last chunk from the session's device arrays straight into the live pre store (positions clipped to 0 ..
 * 2^31 - 1, then what ig_pre_add_pairs does; scalars, ms: as there) or the live pairs session (a position outside 1 .. 2^31 - 1 as 0, a
 * negative id as -1, the strand codes, then what ig_pairs_lift does without its per-pair outputs; scalars: as there).  Refused without
 * the respective live session. */
int ig_text_feed_pre(ig_ctx* ctx, int64_t scalars[8], float* ms);
int ig_text_feed_pairs(ig_ctx* ctx, int64_t scalars[8]);
int ig_text_end(ig_ctx* ctx);

/* ---- the polished FASTA of the polish step: the composition of the input records and the output file stitched from their bases (the
 * rule, stated once: instagraal_amd/scaffold_polish.py).  A SESSION lives between ig_seq_begin and ig_seq_end (ig_destroy
 * frees a live one) on a created handle; it needs no contacts and no state and changes nothing a move reads; no nuisance step or chain
 * may be in flight.  ig_seq_begin takes the layout of ig_pre_begin and refuses what it refuses. */
int ig_seq_begin(ig_ctx* ctx, const uint8_t* seq, int64_t n_bytes, const int64_t* rec_off, const int32_t* rec_len, int32_t n_records);
/* counts[n_records][8]: per record the letters A, C, G, T, N of either case, the other letters, the lower-case letters, all bases.
 * ms (may be NULL): the kernel's time. */
int ig_seq_composition(ig_ctx* ctx, int64_t* counts, float* ms);
/* The plan of the output file.  Output record j: the header literal[hdr_lit[j] .. + hdr_len[j]), then a body of body_len[j] bases, a
 * newline behind every `width` of them and behind the last line; rec_off[n_out + 1]: the file offset of every header, the file's size
 * last; its pieces are piece_first[j] .. piece_first[j + 1] - 1.  Piece p: `length[p]` (1 .. 2^31 - 1) bases from `start[p]` of the
 * input record src[p] (-1: of the literal buffer), as they are (ori[p] == 1) or as their reverse complement (-1; never a literal
 * piece), at the base body[p] of its body.  Refused, naming the record or the piece: a piece outside its source, pieces that do not
 * tile their body in ascending order without gap or overlap, offsets that are not those of the headers, bodies and lines.  An
 * earlier plan of the session and its counts are gone. */
int ig_seq_plan(ig_ctx* ctx, int32_t n_out, int32_t width, const int64_t* rec_off, const int32_t* hdr_len, const int64_t* hdr_lit, const int64_t* body_len,
                const int64_t* piece_first, int64_t n_pieces, const int32_t* src, const int64_t* start, const int64_t* length, const int32_t* ori,
                const int64_t* body, const uint8_t* literal, int64_t n_literal);
/* The bytes first_byte .. first_byte + n_bytes - 1 of the file into out.  first_byte is a multiple of 16; so is n_bytes unless the
 * window ends with the file.  A window that begins where the windows counted so far end (the first: at 0) adds the classes of its
 * body bases to the counts of ig_seq_out_composition; any other is stitched only.  ms (may be NULL): the kernel's time. */
int ig_seq_window(ig_ctx* ctx, int64_t first_byte, int64_t n_bytes, uint8_t* out, float* ms);
/* counts[n_out][8] of the stitched bodies, junctions included (n_counts: the caller's capacity in words): refused until the windows
 * fetched in file order have reached the file's end */
int ig_seq_out_composition(ig_ctx* ctx, int64_t* counts, int64_t n_counts);
int ig_seq_end(ig_ctx* ctx);

/* ---- the contact levels of the pyramid: the level of a contact list (the upper-triangular sum over (min, max), rows and columns
 * ascending, 64-bit sums), the partners of every fragment, and the next level from the current one through a table (the rule, stated
 * once: instagraal_amd/pyramid_levels.py).  A SESSION lives between ig_pyr_begin and ig_pyr_end (ig_destroy frees a
 * live one) on a created handle; it needs no contacts and no state and changes nothing a move reads; no nuisance step or chain may be
 * in flight.  All ids are 0-based.  A sum of 2^31 or more anywhere in a level is refused, naming the pixel; the current level stays.
 *
 * ig_pyr_begin: the level-0 list of n entries over n_frags fragments in file order; it goes to the device in pieces.  Refused, naming
 * the entry: an id outside 0 .. n_frags - 1, a negative count, a count of 2^31 or more.  *is_canonical: every a <= b and the pairs (a,
 * b) strictly ascending: the list is its own level. */
int ig_pyr_begin(ig_ctx* ctx, int32_t n_frags, const int32_t* a, const int32_t* b, const int64_t* count, int64_t n, int32_t* is_canonical);
/* the level of the uploaded list becomes the current level.  ms (may be NULL): the seven passes of the row builder. */
int ig_pyr_matrix(ig_ctx* ctx, int64_t* n_pixels, float* ms);
/* deg[n_frags] of the current level: deg[i] is the number of j with (M + M^T)[i, j] != 0: a stored zero is no partner, a diagonal
 * entry counts once */
int ig_pyr_degrees(ig_ctx* ctx, int32_t* deg);
/* The next level from the current one, which stays on the device: lut[n_old] (n_old: the fragments of the current level) is the new
 * id of every fragment or -1 (destroyed), ascending wherever it is not -1 and below n_new; an entry with a destroyed end is dropped.
 * skip_first (0 or 1): the first entry of the current level -- of the uploaded list, where no level has been made of it: in file order
 * -- is lost (quirk Q-P1 of the binning).  scalars: {entries_in, skipped, dropped_by_lut, entries_kept, pixels, largest_sum, 0, 0}.
 * ms (may be NULL): the seven passes of the row builder. */
int ig_pyr_remap(ig_ctx* ctx, const int32_t* lut, int32_t n_old, int32_t n_new, int32_t skip_first, int64_t* n_pixels, int64_t scalars[8], float* ms);
/* rowptr[n_frags + 1] of the current level (n_rowptr: the caller's capacity) */
int ig_pyr_rows(ig_ctx* ctx, int64_t* rowptr, int64_t n_rowptr);
/* the entries first .. first + n - 1 of the current level as the three int32 rows of the level's matrix: row, column, count */
int ig_pyr_fetch(ig_ctx* ctx, int64_t first, int64_t n, int32_t* row, int32_t* col, int32_t* count);
int ig_pyr_end(ig_ctx* ctx);
/* entries per upload piece of ig_pyr_begin (0: the default): for tests of the upload in pieces */
int ig_debug_pyr_piece(ig_ctx* ctx, int64_t entries);

/* ---- the balancing's rows from a BUILT map (the rule: entries_of_rows, instagraal_amd/balance.py): a second build
 * for the balancer above, not a second balancer.  ig_balance_build_snapshot fills the rows ig_balance_rows / _fetch / _run / _release
 * serve from the handle's snapshot -- what ig_assembly_contacts_build (level 1), ig_assembly_contacts_build_units,
 * ig_assembly_contacts_coarsen or ig_pairs_pixels_build left on the device -- without a pass over the contacts: an entry (u, v, c) with
 * u == v, with v - u < ignore_diags (>= 1) or outside the mode is counted and dropped, every other one is kept as (u, v, c) and (v, u, c).
 * mode: 0 all; 1 cis: group[u] == group[v]; 2 trans: group[u] != group[v]; group: int32 [n_group = the snapshot's units], none
 * negative (NULL at mode 0).  A count is NOT limited to 32 bits; a unit's total is, to 2^53 - 1.  The snapshot stays as it is: a fetch or
 * a coarsening behind this call sees the same bytes.  scalars: within_observed, band_observed, other_observed, kept_observed, entries
 * (2 * kept), entries_in (the snapshot's), n_units, entries_out.  Refused, naming the reason, with nothing built: no snapshot, a level 0
 * snapshot, ignore_diags < 1, a mode outside 0 .. 2, a mode without its groups, a negative group, a nuisance step or a chain in flight, a sharded handle,
 * more than 2^31 - 1 entries, a total of 2^53 or more, rows that do not fit the free device memory beside the snapshot. */
int ig_balance_build_snapshot(ig_ctx* ctx, int32_t ignore_diags, int32_t mode, const int32_t* group, int64_t n_group, int64_t* n_units, int64_t* n_entries,
                              int64_t scalars[8]);
/* tests: the same build over caller CSR data (upper triangular: col >= row, strictly ascending in a row; rowptr [n_rows + 1]) on a bare
 * handle.  The data is checked on the host (a single count of 2^53 or more is refused there: the totals are 64-bit sums), becomes the handle's snapshot (level 2: ig_assembly_contacts_rows / _fetch / _coarsen see it)
 * and the one implementation builds from it. */
int ig_debug_balance_snapshot(ig_ctx* ctx, const int64_t* rowptr, const int32_t* col, const int64_t* count, int64_t n_rows, int32_t ignore_diags, int32_t mode,
                              const int32_t* group, int64_t n_group, int64_t* n_units, int64_t* n_entries, int64_t scalars[8]);
/* the build from the resident snapshot (ignore_diags 2, mode 0) n times, hipEvents around each pass -> ms_n [n][7]: count, rows, scatter,
 * sort_short, sort_lds, sort_long, gather */
int ig_debug_balance_snapshot_time(ig_ctx* ctx, int32_t n, float* ms_n);
#ifdef __cplusplus
}
#endif
#endif
