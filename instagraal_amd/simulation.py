"""From an instaGRAAL input folder to a running sampler and back to `info_frags.txt` / `genome.fasta`: the callers on
either side of the scoring path (reference: simu_single.py "SS" and instagraal.py "IG").

* ``simulation`` mirrors SS:27-175: pyramid (``pyramid.build_and_filter`` with 9 levels of factor 3, SS:539-550), the
  two levels in use, the sub-fragment tables (``create_sub_frags`` SS:674-723, ``create_new_sub_frags`` SS:725-739),
  the structure-of-arrays states with the duplicate-fragment columns (``modify_vect_frags`` SS:221-347: the reference
  hard-wires an empty duplicate list, SS:512, so these only add ``rep / activ / id_d``), the 29 constructor arguments
  of the sampler (SS:120-153) and the initial P(s) estimation (SS:157-171).
* ``instagraal_class.full_em`` mirrors IG:196-291: cycles over shuffled bins, per-cycle outputs
  (``save_simu_step_<j>.txt``, ``info_frags.txt``, ``genome.fasta``, the ``list_*.txt`` traces, with ``save_matrix`` the
  contact map ``matrix_cycle_<j>.png``).  Cycles without
  nuisance sampling run through ``step_sampler_batch`` (the results are identical).
* ``run_instagraal`` mirrors IG:502-581.

``assemble_sampler_args`` needs no GPU and is what the CPU tests pin against the reference's own values.
"""
from __future__ import annotations

import os

import numpy as np

from . import pyramid as pyr

INT2 = np.dtype([("x", np.int32), ("y", np.int32)], align=True)
INT3 = np.dtype([("x", np.int32), ("y", np.int32), ("z", np.int32)], align=True)
INT4 = np.dtype([("x", np.int32), ("y", np.int32), ("z", np.int32), ("w", np.int32)], align=True)
FLOAT3 = np.dtype([("x", np.float32), ("y", np.float32), ("z", np.float32)], align=True)
FLOAT4 = np.dtype([("x", np.float32), ("y", np.float32), ("z", np.float32), ("w", np.float32)], align=True)

SIZE_PYRAMID, FACTOR = 9, 3  # SS:541-542


def _with_duplicate_columns(soa):
    """SS:221-347 / 349-457 without duplicated fragments: the loader's arrays + rep = 0, activ = 1, id_d = id"""
    out = {k: np.array(v, dtype=np.int32) for k, v in soa.items()}
    n = len(out["id"])
    out["rep"] = np.zeros(n, np.int32)
    out["activ"] = np.ones(n, np.int32)
    out["id_d"] = out["id"].copy()
    return out


def _dispatcher(n):
    """SS:312-328 without duplicates: every initial fragment owns one slot"""
    d = np.zeros(n, INT2)
    d["x"] = np.arange(n)
    d["y"] = np.arange(n) + 1
    return np.arange(n, dtype=np.int32), d


def create_sub_frags(spec_level, sub_level_soa):
    """SS:674-723: per bin its <= 3 sub-fragments (ids, lengths in kb, accumulated restriction fragments) and, per
    sub-fragment, (parent bin, Watson offset, Crick offset, index in bin) = distance from either end of the bin to the
    middle of the sub-fragment, accumulated in float32 exactly as the reference does."""
    lo = spec_level["sub_low_index"] - 1
    hi = spec_level["sub_high_index"] - 1
    n = len(lo)
    unkb = np.float32(1000.0)
    len_bp = np.zeros(n, FLOAT3)
    ids = np.zeros(n, INT4)
    accu = np.zeros(n, INT3)
    sub2frag, collect_accu, norm = [], [], []
    for i in range(n):
        n_sub = int(hi[i] - lo[i] + 1)
        v_len = [np.float32(sub_level_soa["len_bp"][lo[i] + j]) / unkb for j in range(n_sub)]
        v_acc = [np.int32(sub_level_soa["n_accu"][lo[i] + j]) for j in range(n_sub)]
        for j, key in zip(range(n_sub), ("x", "y", "z")):
            len_bp[key][i] = v_len[j]
            ids[key][i] = lo[i] + j
            accu[key][i] = v_acc[j]
        ids["w"][i] = n_sub
        collect_accu.extend(v_acc)
        tmp_len = np.array(v_len, dtype=np.float32)
        for j in range(n_sub):
            w_d = np.sum(tmp_len[0:j]) + tmp_len[j] / 2.0
            c_d = np.sum(tmp_len[list(range(n_sub - 1, j, -1))]) + tmp_len[j] / 2.0
            sub2frag.append((i, w_d, c_d, j))
        norm.append(np.sum(v_acc))
    return dict(np_sub_frags_2_frags=np.array(sub2frag, dtype=FLOAT4), np_sub_frags_len_bp=len_bp, np_sub_frags_accu=accu,
                np_sub_frags_id=ids, collect_accu_frags=np.array(collect_accu, dtype=np.float32), norm_vect=np.asmatrix(norm),
                init_n_sub_frags=int(np.sum(hi - lo + 1)))


def assemble_sampler_args(hic_pyr, level, n_iterations=10, is_simu=False, use_rippe=True):
    """The 29 constructor arguments of the sampler (CL:92-125) for resolution `level` of a built pyramid, in order,
    as a dict (vel / pos, OpenGL leftovers, are None).  No GPU involved."""
    lev = hic_pyr.get_level(level)
    sub = hic_pyr.get_level(level - 1)
    spec = hic_pyr.spec_level[str(level)]
    t = create_sub_frags(spec, sub.S_o_A_frags)
    n_frags = lev.n_frags
    new_soa = _with_duplicate_columns(lev.S_o_A_frags)
    new_sub_soa = _with_duplicate_columns(sub.S_o_A_frags)
    collector, dispatcher = _dispatcher(n_frags)
    sub_collector, sub_dispatcher = _dispatcher(len(sub.S_o_A_frags["id"]))
    # create_new_sub_frags SS:725-739: consecutive ids for the sub-fragments of the (possibly duplicated) bins
    rep_ids = np.zeros(n_frags, INT4)
    n_sub = t["np_sub_frags_id"]["w"][new_soa["id_d"]]
    first = np.cumsum(n_sub) - n_sub
    for j, key in enumerate(("x", "y", "z")):
        rep_ids[key] = np.where(n_sub > j, first + j, 0)
    rep_ids["w"] = n_sub
    args = dict(
        use_rippe=use_rippe, S_o_A_frags=new_soa, collector_id_repeats=collector, frag_dispatcher=dispatcher, id_frag_duplicated=[],
        id_frags_blacklisted=[], n_frags=n_frags, n_new_frags=len(new_soa["id"]), init_n_sub_frags=t["init_n_sub_frags"],
        n_new_sub_frags=int(n_sub.sum()), np_rep_sub_frags_id=rep_ids, sub_sampled_sparse_matrix=lev.sparse_mat_csr,
        np_sub_frags_len_bp=t["np_sub_frags_len_bp"], np_sub_frags_id=t["np_sub_frags_id"], np_sub_frags_accu=t["np_sub_frags_accu"],
        np_sub_frags_2_frags=t["np_sub_frags_2_frags"],
        mean_squared_frags_per_bin=np.float32((t["collect_accu_frags"].mean()) ** 2), norm_vect_accu=t["norm_vect"],
        sub_candidates_dup=[], sub_candidates_output_data=[], S_o_A_sub_frags=new_sub_soa, sub_collector_id_repeats=sub_collector,
        sub_frag_dispatcher=sub_dispatcher, sparse_matrix=sub.sparse_mat_csr, mean_value_trans=sub.mean_value_trans,
        n_iterations=n_iterations, is_simu=is_simu, vel=None, pos=None)
    return args, lev, sub


class simulation:
    """SS:27-175 with the MI355X sampler underneath."""

    def __init__(self, name, folder_path, fasta, level, n_iterations, is_simu, use_rippe, thresh_factor=1, output_folder=None,
                 device_id=0):
        from .sampler import sampler as sampler_lib

        self.name = self.data_set = name
        self.use_rippe = use_rippe
        self.str_level, self.str_sub_level = str(level), str(level - 1)
        self.thresh_factor = thresh_factor
        self.fasta = fasta
        self.base_folder = folder_path
        self.output_folder = output_folder if output_folder is not None else os.path.join(os.getcwd(), "results")
        self.n_iterations = n_iterations
        self.select_data_set(name)
        args, self.level, self.sub_level = assemble_sampler_args(self.hic_pyr, level, n_iterations, is_simu, use_rippe)
        self.level.build_seq_per_bin(genome_fasta=self.fasta)
        self.n_frags = args["n_new_frags"]
        self.new_S_o_A_frags, self.new_sub_S_o_A_frags = args["S_o_A_frags"], args["S_o_A_sub_frags"]
        self.sampler = sampler_lib(**args, device_id=device_id, keep_all_scores=False)  # (nobody reads them: CL:1414-1454)
        self.sampler.contig_names = {n: i + 1 for i, n in enumerate(self.hic_pyr.list_contigs_name)}  # (the ids of S_o_A_sub_frags["id_c"]: pairs come by name)
        # SS:157-171
        g = self.sampler.gpu_vect_frags
        g.copy_from_gpu()
        id_start = np.nonzero(g.start_bp == 0)[0]
        max_dist_kb = g.l_cont_bp[id_start].max() / 1000.0
        mean_size_bin_kb = self.new_sub_S_o_A_frags["len_bp"].mean() / 1000.0
        if self.use_rippe and not is_simu:
            self.sampler.estimate_parameters_rippe(max_dist_kb, mean_size_bin_kb / 2.0, False)
        else:
            raise NotImplementedError("only the Rippe model on real data is supported (use_rippe=False is unreachable in the "
                                      "reference as well, SURVEY section 2a)")

    def select_data_set(self, name):  # SS:539-570
        os.makedirs(self.output_folder, exist_ok=True)
        self.hic_pyr = pyr.build_and_filter(self.base_folder, SIZE_PYRAMID, FACTOR, thresh_factor=self.thresh_factor,
                                            output_folder=self.output_folder)
        self.output_folder = os.path.join(self.output_folder, self.data_set, "test_mcmc_" + self.str_level)
        os.makedirs(self.output_folder, exist_ok=True)
        self.new_fasta = os.path.join(self.output_folder, "genome.fasta")
        self.info_frags = os.path.join(self.output_folder, "info_frags.txt")

    def export_new_fasta(self):  # SS:780-782
        self.sampler.gpu_vect_frags.copy_from_gpu()
        self.level.generate_new_fasta(self.sampler.gpu_vect_frags, self.new_fasta, self.info_frags)

    def release(self):
        self.sampler.free_gpu()


class instagraal_class:
    """IG:76-330: the cycle loop and the run's text outputs."""

    TRACES = ("mean_len", "n_contigs", "dist_init_genome", "likelihood", "fact", "slope", "d_max", "d_nuc", "d", "success")

    def __init__(self, name, folder_path, fasta, device, level, n_iterations_em, n_iterations_mcmc, is_simu, scrambled, perform_em,
                 use_rippe, sample_param, thresh_factor, output_folder):
        self.device = device
        self.sample_param = sample_param
        self.simulation = simulation(name, folder_path, fasta, level, n_iterations_em, is_simu, use_rippe, thresh_factor,
                                     output_folder=output_folder, device_id=device)
        self.dt = np.float32(0.01)
        self.collect = {k: [] for k in self.TRACES}
        self.collect_op_sampled, self.collect_id_fA_sampled, self.collect_id_fB_sampled = [], [], []
        self.collect_likelihood_nuisance = []

    def _out(self, name):
        return os.path.join(self.simulation.output_folder, name)

    def _record(self, id_frag, o, dist, op_sampled, id_f_sampled, mean_len, n_contigs):
        c = self.collect
        c["likelihood"].append(o)
        c["n_contigs"].append(n_contigs)
        c["mean_len"].append(mean_len)
        c["dist_init_genome"].append(dist)
        self.collect_op_sampled.append(op_sampled)
        self.collect_id_fB_sampled.append(id_f_sampled)
        self.collect_id_fA_sampled.append(id_frag)

    def full_em(self, n_cycles, n_neighbours, bomb, id_start_sample_param, save_matrix=False, save_law=False, save_junctions=False,
                save_contacts=False, save_joins=False, save_residuals=False, save_placements=False, save_orientations=False, save_weights=False, save_gaps=False,
                save_resolutions=False, save_segment_placements=False, polish=False, save_cut_join=False, pairs=None, save_lifted_pairs=False, balance_pairs=False):  # IG:196-291
        sampler = self.simulation.sampler
        if bomb:
            sampler.bomb_the_genome()
        list_frags = np.arange(0, sampler.n_new_frags)
        t = 0
        n_iter = n_cycles * sampler.n_new_frags
        for j in range(n_cycles):
            np.random.shuffle(list_frags)
            if self.sample_param and j > id_start_sample_param:
                # step_sampler + step_nuisance_parameters per bin (IG:221-252), the two in flight together on the GPU
                res, tuples = sampler.step_sampler_nuisance_batch(list_frags, n_neighbours, self.dt, t, n_iter)
                for id_frag, r, (fact, d, d_max, d_nuc, slope, lik, success, _) in zip(list_frags, res, tuples):
                    self._record(id_frag, float(r["o"]), float(r["dist"]), int(r["op_sampled"]), int(r["id_f_sampled"]),
                                 np.float32(r["mean_len"]), int(r["n_contigs"]))
                    for k, v in (("fact", fact), ("d", d), ("d_max", d_max), ("d_nuc", d_nuc), ("slope", slope), ("success", success)):
                        self.collect[k].append(v)
                    self.collect_likelihood_nuisance.append(lik)
                t += len(list_frags)
            else:  # no nuisance step between the moves: the whole cycle is one batch (same RNG stream, same results)
                res = sampler.step_sampler_batch(list_frags, n_neighbours)
                for id_frag, r in zip(list_frags, res):
                    self._record(id_frag, float(r["o"]), float(r["dist"]), int(r["op_sampled"]), int(r["id_f_sampled"]),
                                 np.float32(r["mean_len"]), int(r["n_contigs"]))
                t += len(list_frags)
            c = sampler.gpu_vect_frags
            c.copy_from_gpu()
            with open(self._out("save_simu_step_%d.txt" % j), "w") as h:
                for pos, start_bp, id_c, ori in zip(c.pos, c.start_bp, c.id_c, c.ori):
                    h.write(str(pos) + "\t" + str(start_bp) + "\t" + str(id_c) + "\t" + str(ori) + "\n")
            self.simulation.export_new_fasta()
            self.save_behaviour_to_txt()
            try:  # IG:278-287
                if save_matrix:
                    sampler.display_current_matrix(self._out("matrix_cycle_%d.png" % j))
            except OSError as e:
                import warnings

                warnings.warn("could not write the matrix at cycle %d: %s" % (j, e))
            if save_law:  # (no reference counterpart: the distance law of the genome behind this cycle)
                from . import distance_law as dlaw

                dlaw.write_law(self._out("distance_law_cycle_%d.txt" % j), sampler.distance_law())
            if save_junctions:  # (no reference counterpart: which joins of this cycle's genome the contacts support)
                from . import junction_profile as jprof

                jprof.write_profile(self._out("junctions_cycle_%d.txt" % j), sampler.junction_profile())
            if save_residuals:  # (no reference counterpart: this cycle's genome against what the model predicts of it)
                from . import expected_map as emap

                res = sampler.display_residual_matrix(self._out("residuals_cycle_%d.png" % j))
                emap.write_residuals(self._out("residuals_cycle_%d.txt" % j), sampler.strongest_residuals(residuals=res), res)
        if polish:  # (once, behind the last cycle and in front of every report below: greedy segment edits, scored exactly)
            from . import rearrange as ra

            every = polish == "all"  # (cuts and joins proposed next to the flips and the moves: DESIGN 4.24)
            ra.write_polish_log(self._out("polish.txt"), sampler.polish(cuts=every, joins=every))
            sampler.gpu_vect_frags.copy_from_gpu()
            self.simulation.export_new_fasta()  # (info_frags.txt and genome.fasta of the polished genome)
        if save_cut_join:  # (once, behind the last cycle and the polishing: the cuts and the links the likelihood would take)
            from . import cut_join as cj

            cj.write_cuts(self._out("cuts.txt"), sampler.weakest_cuts())
            cj.write_links(self._out("links.txt"), sampler.strongest_joins())
        if pairs is not None:  # (once, behind the last cycle and the polishing: the read pairs on the final genome, at bp resolution)
            from . import pairs_lift as pl, zoom_levels as zl

            sampler.pairs_end()
            try:  # (ONE reading of the text, which is what bounds this block: lifted once into one session, everything built from its store)
                if save_lifted_pairs:
                    sampler.write_lifted_pairs(pairs, self._out("lifted.pairs.gz"), keep_session=True)
                else:
                    sampler._pairs_load(pairs)
                sampler.write_pairs_zoom_levels(self._out("pairs_zoom_levels"), None, zl.DEFAULT_RESOLUTIONS if save_resolutions in (False, True) else tuple(save_resolutions),
                                                **(dict(balance=balance_pairs) if balance_pairs else {}))
                law = sampler.pairs_distance_law(None)
                pl.write_law(self._out("pairs_law.txt"), law["counts"], law["edges_bp"])
            finally:
                sampler.pairs_end()
        if save_contacts:  # (once, behind the last cycle: the table is large)
            sampler.write_assembly_contacts(self._out("assembly_contacts"), level="sub")
        if save_resolutions:  # (once, behind the last cycle, beside assembly_contacts/: the fixed-resolution maps and the scaffold matrix)
            from . import zoom_levels as zl

            sampler.write_zoom_levels(self._out("zoom_levels"), zl.DEFAULT_RESOLUTIONS if save_resolutions is True else tuple(save_resolutions),
                                      balance=bool(save_weights))
        if save_joins:  # (once, behind the last cycle: behind a bomb the table has up to four lines per contact)
            from . import join_support as jsup

            jsup.write_joins(self._out("joins.txt"), sampler.join_support())
        if save_placements:  # (once, behind the last cycle, where joins.txt is written: the bins the contacts would rather see elsewhere)
            from . import placement_support as psup

            psup.write_placements(self._out("placements.txt"), sampler.placement_support())
        if save_segment_placements:  # (once, behind the last cycle, next to placements.txt: the blocks, then the scaffolds, the contacts would rather see elsewhere)
            from . import segment_placement as spl

            spl.write_segment_placements(self._out("segment_placements.txt"), sampler.segment_placement(level="block"), title="level=block")
            spl.write_segment_placements(self._out("segment_placements.txt"), sampler.segment_placement(level="scaffold"), mode="a", title="level=scaffold")
        if save_weights:  # (once, behind the last cycle, beside placements.txt: the balancing weight of every bin of the final genome)
            from . import balance as bal

            res = sampler.balance(level="bin")
            bal.write_weights(self._out("weights.txt"), res["bins"], res)
        if save_orientations:  # (once, behind the last cycle: the blocks, then the bins, the contacts would turn round)
            from . import orientation_support as osup

            osup.write_orientations(self._out("orientations.txt"), sampler.orientation_support(level="block"), title="level=block")
            osup.write_orientations(self._out("orientations.txt"), sampler.orientation_support(level="bin"), mode="a", title="level=bin")
        if save_gaps:  # (once, behind the last cycle: the joins between blocks, then between bins, with the gap the contacts put across each)
            from . import gap_support as gsup

            gsup.write_gaps(self._out("gaps.txt"), sampler.gap_support(level="block"), title="level=block")
            gsup.write_gaps(self._out("gaps.txt"), sampler.gap_support(level="bin"), mode="a", title="level=bin")
        self.save_behaviour_to_txt()

    def save_behaviour_to_txt(self):  # IG:293-330
        for k in self.TRACES:
            with open(self._out("list_%s.txt" % k), "w") as h:
                for item in self.collect[k]:
                    h.write("%s\n" % item)
        with open(self._out("list_mutations.txt"), "w") as h:
            h.write("id_fA\tid_fB\tid_mutation\n")
            for a, b, m in zip(self.collect_id_fA_sampled, self.collect_id_fB_sampled, self.collect_op_sampled):
                h.write("%s\t%s\t%s\n" % (a, b, m))


def run_instagraal(hic_folder, reference_fa, output_folder=None, level=4, cycles=100, coverage_std=1, neighborhood=5, device=0,
                   circular=False, bomb=False, pyramid_only=False, save_pickle=False, save_matrix=False, simple=False, save_law=False,
                   save_junctions=False, save_contacts=False, save_joins=False, save_residuals=False, save_placements=False,
                   save_orientations=False, save_weights=False, save_gaps=False, save_resolutions=False, save_segment_placements=False, polish=False,
                   save_cut_join=False, pairs=None, save_lifted_pairs=False):
    """IG:502-581 (defaults of cli/main.py: level 4, 100 cycles, 5 neighbours, 1 std).  The three trailing switches of the
    reference's signature (IG:512-514) are accepted: ``save_pickle`` dumps the run object to ``graal.pkl`` as the reference
    tries to (IG:589-594: a warning when it cannot be pickled -- device handles here, h5py handles there); ``save_matrix``
    writes the contact map of the genome after every cycle to ``matrix_cycle_<j>.png`` (``display_current_matrix``, IG:279-284;
    built on the GPU, binned to at most 2048 pixels a side: DESIGN 4.10); ``simple`` calls ``instagraal_class.simple_start``, a
    method the reference does not define (IG:582 raises AttributeError): refused.  ``save_law`` (an addition: the reference has
    nothing like it) writes the distance law of the genome after every cycle to ``distance_law_cycle_<j>.txt`` (columns edge_lo,
    edge_hi, observed, pairs: ``sampler.distance_law``); ``save_junctions`` (an addition too) writes the junction support
    profile of that genome to ``junctions_cycle_<j>.txt``: one line per join between two bins of a contig with the contacts observed
    across it inside a window of 64 sub-fragments, the pairs, the model's expectation and their ratio
    (``sampler.junction_profile``); ``save_contacts`` (an addition as well) writes the contacts in the coordinates of the
    final genome once, behind the last cycle, to ``assembly_contacts/bins.bed``, ``pixels.tsv`` and ``chrom.sizes`` -- sub-fragment
    resolution, sorted, upper-triangular: what ``cooler load -f coo bins.bed pixels.tsv`` takes -- with the scaffold names of
    ``genome.fasta`` (``sampler.write_assembly_contacts``; not per cycle: the table has one line per contact);
    ``save_joins`` (an addition too) writes ``joins.txt`` once, behind the last cycle: one line per pair of scaffold ends that the
    contacts link inside a window of 64 sub-fragments -- the joins the sampler did not make -- with the contacts observed, the pairs,
    the model's expectation and their ratio (``sampler.join_support``); ``save_residuals`` (an addition too) writes after
    every cycle ``residuals_cycle_<j>.png``, log2(observed / expected) of that genome's contact map against what the model in use
    predicts for every pixel, and ``residuals_cycle_<j>.txt``, the 20 pixels off the diagonal with the largest excess
    (``sampler.residual_map``, ``sampler.strongest_residuals``); ``save_placements`` (an addition too) writes
    ``placements.txt`` once, behind the last cycle: one line per bin whose contacts are denser around another site of the genome than
    around where it sits, inside a window of 64 sub-fragments, with that site, the two densities and their ratio
    (``sampler.placement_support``); ``save_orientations`` (an addition too) writes ``orientations.txt`` once, behind the
    last cycle: one line per judged segment -- the co-linear blocks first, the bins behind them -- with the contacts between its two
    ends and the positions on either side inside a window of 8 sub-fragments, split into those that keep it as it lies and those that
    would reverse it (``sampler.orientation_support``); ``save_weights`` (an addition too) writes ``weights.txt`` once, behind
    the last cycle: one line per bin of the final genome with its scaffold, start, end and balancing weight -- the raw count of two bins
    times their two weights is the balanced count (``sampler.balance``); ``save_gaps`` (an addition too) writes ``gaps.txt``
    once, behind the last cycle: one line per join -- those between two co-linear blocks of a scaffold first, those between two bins
    behind them -- with the contacts observed across it inside a window of 64 sub-fragments, the pairs, the gap in kb under which the
    model explains them best, its 95 % interval, the two log-likelihood ratios and the verdict "adjacent", "gap" or "apart"
    (``sampler.gap_support``); ``save_resolutions`` (an addition too; True: ``zoom_levels.DEFAULT_RESOLUTIONS``, or a tuple
    of ascending bin sizes in bp) writes ``zoom_levels/`` once, behind the last cycle, beside ``assembly_contacts/``: per bin size
    ``resolutions/<bp>/bins.bed``, ``pixels.tsv`` and ``chrom.sizes`` -- the contacts of the final genome in fixed bins of that many bp,
    a level whose bin size is a multiple of the one before it made from that level alone -- and ``scaffolds/`` with the scaffold by
    scaffold matrix; given together with ``save_weights``, ``weights.tsv`` of every level beside them (``sampler.write_zoom_levels``,
    DESIGN 4.21); ``save_segment_placements`` (an addition too) writes ``segment_placements.txt`` once, behind the last cycle, next to
    ``placements.txt``: one line per segment -- the co-linear blocks first, the whole scaffolds behind them -- whose contacts are denser
    around another site of the genome than around where it lies, with that site, the two densities, their ratio and the way round the
    contacts would put it in there (``sampler.segment_placement``); ``polish`` (an addition too) runs ``sampler.polish``
    once, behind the last cycle and in front of every ``save_*`` report that is written once: greedy segment edits proposed by the
    block-level reports and scored exactly, logged to ``polish.txt`` (round, edit, delta, likelihood); ``info_frags.txt``,
    ``genome.fasta`` and those reports then describe the polished genome (``rearrange.py``); ``polish="all"`` also proposes
    the weakest cuts and the strongest joins (``cut_join.py``); ``save_cut_join`` (an addition too) writes ``cuts.txt`` and ``links.txt``
    once, behind the last cycle and the polishing: the cuts and the links with the largest positive likelihood change, each with its
    edit (``sampler.weakest_cuts``, ``sampler.strongest_joins``); ``pairs`` (an addition too: the path of the 4DN pairs file the
    contacts came from, aligned to the input contigs) writes once, behind the last cycle and any polishing, ``pairs_zoom_levels/`` -- the
    folders of ``zoom_levels/`` built from the read pairs lifted onto the final genome, a pair counted where it falls (bin sizes:
    ``save_resolutions`` where it is a tuple, else the defaults) -- and ``pairs_law.txt``, their distance histogram per strand
    combination; with ``save_lifted_pairs`` also ``lifted.pairs.gz``, the pairs file in the coordinates of ``genome.fasta``
    (``sampler.write_pairs_zoom_levels``, ``sampler.pairs_distance_law``, ``sampler.write_lifted_pairs``); the balancing
    weights of those levels are ``run_balanced_pairs``' (this function's signature stays as it is)."""
    return _run_instagraal(hic_folder, reference_fa, output_folder=output_folder, level=level, cycles=cycles, coverage_std=coverage_std, neighborhood=neighborhood,
                           device=device, circular=circular, bomb=bomb, pyramid_only=pyramid_only, save_pickle=save_pickle, save_matrix=save_matrix, simple=simple,
                           save_law=save_law, save_junctions=save_junctions, save_contacts=save_contacts, save_joins=save_joins, save_residuals=save_residuals,
                           save_placements=save_placements, save_orientations=save_orientations, save_weights=save_weights, save_gaps=save_gaps,
                           save_resolutions=save_resolutions, save_segment_placements=save_segment_placements, polish=polish, save_cut_join=save_cut_join, pairs=pairs,
                           save_lifted_pairs=save_lifted_pairs)


def _run_instagraal(hic_folder, reference_fa, output_folder=None, level=4, cycles=100, coverage_std=1, neighborhood=5, device=0,
                    circular=False, bomb=False, pyramid_only=False, save_pickle=False, save_matrix=False, simple=False, save_law=False,
                    save_junctions=False, save_contacts=False, save_joins=False, save_residuals=False, save_placements=False,
                    save_orientations=False, save_weights=False, save_gaps=False, save_resolutions=False, save_segment_placements=False, polish=False,
                    save_cut_join=False, pairs=None, save_lifted_pairs=False, balance_pairs=False):
    """``run_instagraal``'s body, with the one keyword its pinned signature does not have: ``balance_pairs`` (``full_em``)"""
    import warnings

    if simple and not pyramid_only:
        raise NotImplementedError("simple=True: the reference calls instagraal_class.simple_start (instagraal.py:582), which it does not define")
    name = os.path.basename(os.path.normpath(str(hic_folder)))
    if pyramid_only:
        root = str(output_folder) if output_folder is not None else os.path.join(os.getcwd(), "results")
        os.makedirs(root, exist_ok=True)
        return pyr.build_and_filter(str(hic_folder), SIZE_PYRAMID, FACTOR, thresh_factor=coverage_std, output_folder=root)
    p2 = instagraal_class(name=name, folder_path=str(hic_folder), fasta=str(reference_fa), device=device, level=level,
                          n_iterations_em=30, n_iterations_mcmc=100, is_simu=False, scrambled=False, perform_em=False, use_rippe=True,
                          sample_param=True, thresh_factor=coverage_std, output_folder=str(output_folder) if output_folder else None)
    if circular:
        # IG:569-570: the flag is applied to the loader's arrays AFTER the sampler copied them to the device, i.e. it
        # has no effect on the run in the reference either (quirk Q14).  Accepted and applied the same (ineffective) way.
        warnings.warn("--circular has no effect on the assembly (as in the reference: instagraal.py:569-570 sets the flag "
                      "after the sampler copied the fragment arrays)")
        p2.simulation.level.S_o_A_frags["circ"] += 1
    p2.full_em(n_cycles=cycles, n_neighbours=neighborhood, bomb=bomb, id_start_sample_param=4, save_matrix=save_matrix, save_law=save_law,
               save_junctions=save_junctions, save_contacts=save_contacts, save_joins=save_joins, save_residuals=save_residuals, save_placements=save_placements,
               save_orientations=save_orientations, save_weights=save_weights, save_gaps=save_gaps, save_resolutions=save_resolutions,
               save_segment_placements=save_segment_placements, polish=polish, save_cut_join=save_cut_join, pairs=pairs, save_lifted_pairs=save_lifted_pairs,
               balance_pairs=balance_pairs)
    if save_pickle:  # IG:589-594
        import pickle

        try:
            with open("graal.pkl", "wb") as h:
                pickle.dump(p2, h)
        except Exception as e:  # ctypes handles do not pickle (the reference: h5py handles)
            warnings.warn("could not pickle the run state: %s" % (e,))
            try:
                os.remove("graal.pkl")
            except OSError:
                pass
    return p2


def run_from_pairs(fasta, pairs, enzymes, output_folder, **run_kw):
    """FASTA + 4DN pairs -> assembly: ``pre.run_pre`` writes the three input files into ``<output_folder>/pre/`` (the digest, G+C and
    the pixels on the device: DESIGN 4.26; the keyword ``reader`` is ``pre.run_pre_reader``'s, "host" or "device": who parses the pairs text), then
    ``run_instagraal`` runs on that folder unchanged with ``fasta`` as the reference and ``run_kw`` as its keywords.  Returns what
    ``run_instagraal`` returns."""
    from . import pre

    folder = os.path.join(str(output_folder), "pre")
    pre.run_pre_reader(fasta, pairs, enzymes, folder, reader=run_kw.pop("reader", "host"))
    return run_instagraal(folder, str(fasta), output_folder=str(output_folder), **run_kw)


def run_balanced_pairs(hic_folder, reference_fa, pairs, output_folder=None, balance_pairs=True, **run_kw):
    """``run_instagraal(..., pairs=pairs)`` with the balancing weights of the read-pair maps: ``balance_pairs`` (True, or a
    dict of ``sampler.pairs_balance``'s parameters such as ``mode="cis"``) writes ``weights.tsv`` beside the pixels of every level of
    ``pairs_zoom_levels/`` (``sampler.write_pairs_zoom_levels(balance=...)``), as the reference's ``post`` ends with ``cooler balance`` on
    every zoom level; False: this IS ``run_instagraal``, the same files and bytes.  Returns what ``run_instagraal`` returns."""
    return _run_instagraal(hic_folder, reference_fa, output_folder=output_folder, pairs=pairs, balance_pairs=balance_pairs, **run_kw)


def run_device_pyramid(hic_folder, reference_fa, output_folder=None, **run_kw):
    """``run_instagraal`` with the pyramid's contact levels built on the device first:
    ``pyramid_device.build_and_filter`` writes the pyramid where ``run_instagraal`` will look for it -- the same folders, byte for
    byte -- with ``coverage_std`` and ``device`` taken from ``run_kw``; ``run_instagraal`` then runs unchanged, finds every level
    present and rebuilds none.  FASTA + pairs: ``pre.run_pre`` followed by this.  Returns what ``run_instagraal`` returns."""
    from . import pyramid_device

    root = str(output_folder) if output_folder else os.path.join(os.getcwd(), "results")
    os.makedirs(root, exist_ok=True)
    device = run_kw.get("device", 0)
    hic_pyr = pyramid_device.build_and_filter(str(hic_folder), SIZE_PYRAMID, FACTOR, thresh_factor=run_kw.get("coverage_std", 1), output_folder=root,
                                              device=True if device is None or isinstance(device, bool) else device)
    hic_pyr.close()
    return run_instagraal(hic_folder, reference_fa, output_folder=output_folder, **run_kw)


def run_and_polish(hic_folder, reference_fa, output_folder=None, post_polish=False, stats=False, junction="", lost="reference", **run_kw):
    """``run_instagraal`` with the reference's polish step and its statistics behind it; both switches default to off, and
    with both off this IS ``run_instagraal``: the same files, the same output.  ``post_polish`` runs ``scaffold_polish.polish_assembly`` in
    its polishing mode on the run's final ``info_frags.txt`` and ``reference_fa`` into ``<run folder>/polished/`` (``junction``, ``lost``:
    its arguments; the FASTA is stitched on the run's device).  ``stats`` writes ``assembly_stats_comparison.txt`` into the run folder and
    prints it: the comparison table of the input, ``genome.fasta`` and, with ``post_polish``, the polished genome.  Returns what
    ``run_instagraal`` returns; the polish's result is its ``polish_result``."""
    p2 = run_instagraal(hic_folder, reference_fa, output_folder=output_folder, **run_kw)
    if run_kw.get("pyramid_only") or not (post_polish or stats):
        return p2
    from . import assembly_stats, scaffold_polish

    sim = p2.simulation
    folder = sim.output_folder
    results = {"input": assembly_stats.compute_assembly_stats(str(reference_fa)), "genome.fasta": assembly_stats.compute_assembly_stats(sim.new_fasta)}
    if post_polish:
        p2.polish_result = scaffold_polish.polish_assembly(sim.info_frags, str(reference_fa), os.path.join(folder, "polished"), mode="polishing", junction=junction, lost=lost,
                                                           device=True, device_id=run_kw.get("device", 0))
        results["polished"] = p2.polish_result["stats"]["polished"]
    if stats:
        text = assembly_stats.format_comparison_table(results)
        with open(os.path.join(folder, "assembly_stats_comparison.txt"), "w") as h:
            h.write(text)
        print(text)
    return p2
