/*
 * ig_hip.hip -- MI355X (gfx950) implementation of instaGRAAL's per-move scoring path behind the
 * C ABI of include/instagraal_hip.h.  Design notes: DESIGN.md.  Reference being replaced:
 *   /root/reference/src/instagraal/kernels/kernel_sparse_adapt.cu  ("KA", 38 CUDA kernels)
 *   /root/reference/src/instagraal/cuda_lib_gl_single.py           ("CL", pycuda host code)
 *
 * One translation unit; the device code lives in the ig_kernels_*.cuh parts included below, the host side (handles, uploads, the
 * launch sequences, the extern "C" entry points) in the ig_host_*.inc parts: core, upload; genome and rows, the layers the reports
 * on the current genome share; map, law, junc, lift, join, emap, place, orient, bal, gap, one per report; edit, the segment edits; cutjoin, the cut and join scores; pairs, the read pairs lifted onto the genome; pre, the input folder from a FASTA and read pairs; seq, the polished FASTA of the polish step; text, 4DN pairs text parsed on the device; pyr, the pyramid's levels; balsnap, the balancing's rows from a built map; batch, nuis, debug.
 *
 * A batch of W moves (CL:1401-1465 each) is one launch sequence on one stream, no host round trip inside:
 *   k_gather        O(N)            local fragment lists of the touched contigs, uniq-mutation lists, flags
 *   k_mutate        W x C x 25 WGs  one candidate genome per workgroup, operators applied in place on the local window,
 *                                   coordinate columns + zero-pixel sums
 *   k_offsets       1 workgroup     slice-list starts in the pool
 *   k_slice         row-parallel    CSR rows of the touched contigs -> compacted slice lists (every touched contig's rows once per move slot)
 *   k_screen_tail   the hot kernel  two tiers, first: every (contact, column) term in float with a rigorous bound; its first
 *                                   workgroups: quirk Q5, the last S_c mod 64 contacts of every list (k_tail on a second
 *                                   stream where a batch is not screened)
 *   k_contend, k_worklist           the columns that can still win, and their work items
 *   k_score_list    exact           one exact Rippe/Poisson term per (contact, column), 64-bit integer sums: contenders only
 *   k_records, k_predict, k_delta   slot-major score records; predicted windowed winners and their exact deltas
 *   k_decide_batch  1 wave          in-order decisions with the live scalars
 *   k_commit_batch  1 workgroup     winners applied together, exact genome-distance deltas, result records
 * plus the one-move kernels k_scores / k_delta / k_apply / k_post / k_commit (single moves, windowed winners), and the
 * from-scratch pass over all contacts: k_pack_tab_sig / k_nuis_prepare, k_tile_trans, k_full_nz_tiled; the
 * nuisance step's screened pass: k_hist_build / k_hist_walk / k_hist_eval (tier 0), k_full_diff_tiled (tier 1);
 * the reports on the current genome and the three homes of what they share -- the wave idioms: device helpers, no
 * kernel (ig_kernels_wave.cuh); the genome view: k_map_pixels, k_law_records,
 * k_law_sorted; the row builder: k_scan64_totals / _tops / _apply, k_lift_classify, k_lift_sort_wave / _lds, k_lift_merge,
 * k_lift_row_bits, k_lift_head_totals, k_lift_reduce (and the tests' k_debug_rows_emit, k_debug_wave_runs) --; the contact map: k_contact_map, k_map_mirror; the distance
 * law: k_law_observed, k_law_pairs (4.11); the junction support profile: k_junc_observed, k_junc_count, k_junc_model (4.12); the
 * contacts in genome coordinates: k_lift_heads, k_lift_keys, k_lift_pass (4.13); the join support of the scaffold ends: k_join_heads,
 * k_join_ends, k_join_records, k_join_emit, k_join_model (4.14); the expected contact map: k_emap_count, k_emap_rows, k_emap_list,
 * k_emap_tiles, with the mirror of 4.10 (4.15); the placement support of the bins: k_place_bins, k_place_emit, k_place_scan, with the
 * records of 4.14 (4.16); the orientation support of the segments: k_orient_segments, k_orient_paint, k_orient_observed,
 * k_orient_model (4.18); the balancing weights: k_bal_emit, k_bal_marginals, k_bal_mean, k_bal_update, k_bal_var, with the units of
 * 4.13 (4.19); the gap support of the joins: k_gap_junctions, k_gap_paint, k_gap_observed, k_gap_model (4.20); the segment edits: k_edit_plan, k_edit_state, k_edit_delta,
 * k_edit_zero_delta, k_edit_commit (4.23); the cut and join scores: k_cut_span, k_cut_zero, k_cj_vk, k_cj_pairs_emit, k_cj_join,
 * k_cj_contig_zero, k_cj_join_zero (4.24); the read pairs lifted onto the genome: k_pairs_lift, k_pairs_emit, k_pairs_law (4.25); the input
 * folder from a FASTA and read pairs: k_pre_sites, k_pre_marks, k_pre_popc, k_pre_cuts, k_pre_frags, k_pre_assign, k_pre_emit (4.26); the polished FASTA
 * of the polish step: k_seq_composition, k_seq_stitch (4.27); 4DN pairs text: k_text_mark, k_text_lines, k_text_parse, k_text_compact, k_text_convert (4.30); the balancing's rows from a built map: k_balsnap_emit, k_balsnap_gather (4.29).
 *
 * Environment knobs (tests, fault injection and tuning only; the table in INTEGRATION.md section 4 is the reference): IG_BATCH_W, IG_WINDOW
 * (widths), IG_POOL_ENTRIES, IG_WIDE_LISTS, IG_NO_HOST_FLAG, IG_POISON_ALLOC / IG_POISON_ONLY (force the rare paths), IG_SCREEN,
 * IG_SCREEN_VERIFY, IG_ABLATE, IG_WINDOW_CHECK, IG_FUSED_COMMIT, IG_STEP_DRAW_FAST (the same results another way: what the
 * path-against-path tests and fuzzers toggle), IG_NUIS_W, IG_NUIS_SCREEN, IG_NUIS_HIST, IG_NUIS_SCREEN_VERIFY, IG_NUIS_SCREEN_NOCHECK,
 * IG_NUIS_HIST_TRACE, IG_NUIS_CHAIN, IG_NUIS_ASYNC (the nuisance step's tiers and its helper thread).
 */
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <thread>

#include "ig_common.cuh"
#include "ig_model.cuh"
#include "ig_kernels_setup.cuh"
#include "ig_kernels_score.cuh"
#include "ig_kernels_screen.cuh"
#include "ig_kernels_commit.cuh"
#include "ig_kernels_nuis.cuh"
#include "ig_kernels_wave.cuh"
#include "ig_kernels_genome.cuh"
#include "ig_kernels_rows.cuh"
#include "ig_kernels_map.cuh"
#include "ig_kernels_law.cuh"
#include "ig_kernels_junc.cuh"
#include "ig_kernels_lift.cuh"
#include "ig_kernels_join.cuh"
#include "ig_kernels_emap.cuh"
#include "ig_kernels_place.cuh"
#include "ig_kernels_orient.cuh"
#include "ig_kernels_bal.cuh"
#include "ig_kernels_gap.cuh"
#include "ig_kernels_zoom.cuh"
#include "ig_kernels_segplace.cuh"
#include "ig_kernels_edit.cuh"
#include "ig_kernels_cutjoin.cuh"
#include "ig_kernels_pairs.cuh"
#include "ig_kernels_pre.cuh"
#include "ig_kernels_seq.cuh"
#include "ig_kernels_text.cuh"
#include "ig_kernels_pyr.cuh"
#include "ig_kernels_balsnap.cuh"

/* ================================================================== host side (one translation unit, twenty-seven parts) */
#include "ig_host_core.inc"
#include "ig_host_upload.inc"
#include "ig_host_genome.inc"
#include "ig_host_rows.inc"
#include "ig_host_map.inc"
#include "ig_host_law.inc"
#include "ig_host_junc.inc"
#include "ig_host_lift.inc"
#include "ig_host_join.inc"
#include "ig_host_emap.inc"
#include "ig_host_place.inc"
#include "ig_host_orient.inc"
#include "ig_host_bal.inc"
#include "ig_host_gap.inc"
#include "ig_host_zoom.inc"
#include "ig_host_segplace.inc"
#include "ig_host_edit.inc"
#include "ig_host_cutjoin.inc"
#include "ig_host_pairs.inc"
#include "ig_host_pre.inc"
#include "ig_host_seq.inc"
#include "ig_host_text.inc"
#include "ig_host_pyr.inc"
#include "ig_host_balsnap.inc"
#include "ig_host_batch.inc"
#include "ig_host_nuis.inc"
#include "ig_host_debug.inc"
