"""Host-side mirror of the reference's ``sampler`` over the HIP C ABI (drop-in for the scoring path).

Mirrors ``/root/reference/src/instagraal/cuda_lib_gl_single.py`` ("CL"): same constructor
arguments (CL:92-125), same public methods and attributes that ``simulation`` and
``instagraal_class.full_em`` touch:

    step_sampler(id_frag, n_neighbours, dt) -> 6-tuple            CL:1401-1465
    step_nuisance_parameters(dt, t, n_step) -> 8-tuple            CL:2961-3051
    estimate_parameters_rippe / eval_likelihood_init              CL:2239-2372, 1193-1243
    bomb_the_genome, modify_gl_cuda_buffer, dist_inter_genome     CL:1925-1948, 2715-2881, 665-716
    apply_replay_simu, free_gpu                                   CL:2546-2553, 3167-3177
    display_current_matrix(filename) -> 3-tuple, contact_map      CL:2555-2606
    gpu_vect_frags.copy_from_gpu() + numpy attributes             gpustruct.py:162-186

What the reference does with ~450 synchronous pycuda launches and 5 PCIe sorts per move is ONE
call here (``ig_step``: eight launches, one 80-byte D2H).  ``step_sampler_batch`` enqueues many
moves without any host round trip; candidate draws do not depend on the genome state
(CL:3103-3141 reads fixed distributions), so they can be drawn ahead with the same RNG stream.
"""
from __future__ import annotations

import numpy as np

from . import hip_lib
from . import optim_rippe_curve_update as opti
from . import zoom_levels as _zoom_levels

LIST_SIZE = np.array([1, 3, 5, 10, 20, 50, 200, 200], dtype=np.int32)  # CL:417
N_INSERT_BLOCKS = 6  # CL:192
N_TMP_STRUCT = 24  # CL:194
PARAM_NAMES = ("kuhn", "lm", "c1", "slope", "d", "d_max", "fact", "v_inter")  # KA:91-100
PARAM_DTYPE = np.dtype([(k, np.float32) for k in PARAM_NAMES], align=True)  # CL:235-247


def soa17_from_dict(S_o_A_frags, n):
    """17 x N int32 in KA:40-58 order; ``ori`` starts at +1 like create_gpu_struct (CL:537-541)."""
    out = np.zeros((17, n), np.int32)
    for k, name in enumerate(hip_lib.FRAG_FIELDS):
        if name == "ori":
            out[k] = 1
        elif name == "id":
            out[k] = np.arange(n)
        else:
            out[k] = S_o_A_frags[name]
    return out


def estimate_rippe_host(sparse_matrix, np_sub_frags_2_frags, S_o_A_frags, n_frags, mean_value_trans, max_dist_kb, size_bin_kb):
    """Host part of estimate_parameters_rippe (CL:2239-2341), vectorised: for the first n_frags // 10 sub-fragment rows
    whose contig is longer than one bin, the cis contacts are binned by genomic distance (zeros included: every such
    row contributes one value per bin, CL:2289-2292); the per-bin means (+ the trans level) are fitted with
    optim_rippe_curve_update.estimate_param_rippe; the trans level is then lowered tenfold (CL:2338) before the
    cis/trans cut-off is solved.  -> (bins_upd, mean_contacts_upd, p, y_estim, mean_value_trans / 10, d_max)"""
    bins = np.arange(size_bin_kb, max_dist_kb + size_bin_kb, size_bin_kb)
    nb = len(bins)
    sm = sparse_matrix.tocsr()
    parent = np_sub_frags_2_frags["x"].astype(np.int64)
    id_c = S_o_A_frags["id_c"][parent]
    s_all = S_o_A_frags["start_bp"][parent] / 1000.0 + np_sub_frags_2_frags["y"]
    len_kb = S_o_A_frags["l_cont_bp"][parent] / 1000
    acc = np.zeros(nb, np.float64)
    rows = 0
    for i in range(0, int(n_frags) // 10):
        if not (size_bin_kb < len_kb[i]):
            continue
        s, e = sm.indptr[i], sm.indptr[i + 1]
        j, dat = sm.indices[s:e], sm.data[s:e]
        keep = id_c[j] == id_c[i]
        d = np.abs(s_all[i] - s_all[j[keep]])
        ok = d < max_dist_kb
        acc += np.bincount((d[ok] / size_bin_kb).astype(np.int64), weights=dat[keep][ok], minlength=nb)[:nb]
        rows += 1
    mean = acc / max(rows, 1)
    mean_contacts = np.where((rows == 0) | (mean == 0), np.nan, mean + mean_value_trans).astype(np.float32)
    good = ~np.isnan(mean_contacts)
    bins_upd = np.array(bins[good])
    mean_contacts_upd = np.array(mean_contacts[good])
    p, y_estim = opti.estimate_param_rippe(mean_contacts_upd, bins_upd)
    mvt = mean_value_trans / 10.0  # CL:2338
    return bins_upd, mean_contacts_upd, p, y_estim, mvt, opti.estimate_max_dist_intra(p, mvt)


def fit_law(law, mean_value_trans):
    """The fit of ``estimate_rippe_host`` (its last lines) on a law of the current genome (``distance_law.law_host`` or the
    device's): x = the upper edges of the bins, as there; y = observed / pairs + the trans level for the bins whose mean is not
    zero.  -> (bins_upd, mean_contacts_upd, p, y_estim, mean_value_trans / 10, d_max)"""
    from .distance_law import mean_per_pair

    bins = np.asarray(law["edges"][1:], np.float64)
    mean = mean_per_pair(law)
    mean_contacts = np.where(np.isnan(mean) | (mean == 0), np.nan, mean + mean_value_trans).astype(np.float32)
    good = ~np.isnan(mean_contacts)
    bins_upd = np.array(bins[good])
    mean_contacts_upd = np.array(mean_contacts[good])
    p, y_estim = opti.estimate_param_rippe(mean_contacts_upd, bins_upd)
    mvt = mean_value_trans / 10.0  # CL:2338
    return bins_upd, mean_contacts_upd, p, y_estim, mvt, opti.estimate_max_dist_intra(p, mvt)


def problem_to_context(prob, params=None, device_id=0, rank=0, world=1):
    """Upload a synth.SynthProblem (contacts, sub-fragment table, state, fixed parameters)."""
    ctx = hip_lib.Context(device_id)
    ctx.upload_subfrag_table(prob.np_sub_frags_2_frags)
    ctx.upload_contacts(prob.coo_row, prob.coo_col, prob.coo_cnt, prob.n_sub_frags, rank, world)
    max_bounds = LIST_SIZE[:N_INSERT_BLOCKS].max() * np.int32(np.round(prob.S_o_A_frags["sub_len"].mean()) + 1)  # CL:418-420
    ctx.set_insert_config(LIST_SIZE[:N_INSERT_BLOCKS], int(max_bounds))
    ctx.upload_state(soa17_from_dict(prob.S_o_A_frags, prob.n_frags))
    p = prob.params if params is None else params
    mean_kb = np.float32(prob.S_o_A_sub_frags["len_bp"].mean() / 1000.0)  # CL:231, 1120
    ctx.set_params([np.float32(p[k]) for k in PARAM_NAMES], mean_kb, 0)
    ctx.set_params([np.float32(p[k]) for k in PARAM_NAMES], mean_kb, 1)
    return ctx


class DeviceFrags:
    """Stand-in for GPUStruct (gpustruct.py): ``copy_from_gpu()`` refreshes numpy attributes
    ``pos, sub_pos, id_c, ...`` from the device (contig ids canonically renumbered)."""

    def __init__(self, ctx):
        self._ctx = ctx
        self.copy_from_gpu()

    def copy_from_gpu(self, skip=None):
        soa = self._ctx.download_state()
        for k, name in enumerate(hip_lib.FRAG_FIELDS):
            setattr(self, name, soa[k].copy())
        return self

    def soa17(self):
        return np.stack([getattr(self, k) for k in hip_lib.FRAG_FIELDS]).astype(np.int32)


class sampler:  # noqa: N801 - the reference's class name
    def __init__(self, use_rippe, S_o_A_frags, collector_id_repeats, frag_dispatcher, id_frag_duplicated,
                 id_frags_blacklisted, n_frags, n_new_frags, init_n_sub_frags, n_new_sub_frags, np_rep_sub_frags_id,
                 sub_sampled_sparse_matrix, np_sub_frags_len_bp, np_sub_frags_id, np_sub_frags_accu, np_sub_frags_2_frags,
                 mean_squared_frags_per_bin, norm_vect_accu, sub_candidates_dup, sub_candidates_output_data,
                 S_o_A_sub_frags, sub_collector_id_repeats, sub_frag_dispatcher, sparse_matrix, mean_value_trans,
                 n_iterations, is_simu, vel=None, pos=None, device_id=0, coo=None, keep_all_scores=True):
        if not use_rippe:
            raise NotImplementedError("use_rippe=False is unreachable from the reference CLI (instagraal.py:564)")
        if len(sub_candidates_dup) or len(id_frag_duplicated):
            raise NotImplementedError("repeated fragments are dead in the reference (simu_single.py:513)")
        self.o = 0
        self.log_e = 0.43429448190325182  # CL:128
        self.n_frags = np.int32(n_frags)
        self.n_new_frags = np.int32(n_new_frags)
        self.init_n_sub_frags = np.int32(init_n_sub_frags)
        self.n_new_sub_frags = np.int32(n_new_sub_frags)
        self.id_frags_blacklisted = list(id_frags_blacklisted)
        self.S_o_A_frags = S_o_A_frags
        self.S_o_A_sub_frags = S_o_A_sub_frags
        self.np_sub_frags_id = np_sub_frags_id
        self.np_sub_frags_2_frags = np_sub_frags_2_frags
        self.sub_sampled_sparse_matrix = sub_sampled_sparse_matrix
        self.mean_len_bp_frags = S_o_A_sub_frags["len_bp"].mean()  # CL:231
        self.mean_value_trans = mean_value_trans
        self.n_iterations = n_iterations
        self.is_simu = is_simu
        self.dt = np.float32(0.01)
        self.n_insert_blocks = N_INSERT_BLOCKS
        self.n_tmp_struct = N_TMP_STRUCT
        N, M = int(n_new_frags), int(n_new_sub_frags)

        # contacts: CL:129, 564-615 (symmetrise, strict upper triangle, COO row-major)
        if coo is None:
            import scipy.sparse as sp

            self.sparse_matrix = sparse_matrix + sparse_matrix.transpose()
            c = sp.triu(self.sparse_matrix.tocoo(), k=1, format="coo")
            order = np.lexsort((c.col, c.row))
            row, col, dat = c.row[order], c.col[order], c.data[order]
        else:
            row, col, dat = coo
            self.sparse_matrix = None
        self.n_non_zero = int(len(dat))

        self.ctx = hip_lib.Context(device_id)
        self.ctx.upload_subfrag_table(np_sub_frags_2_frags)
        self.ctx.upload_contacts(row, col, dat, M)
        self.max_bounds_insert = LIST_SIZE[:N_INSERT_BLOCKS].max() * np.int32(np.round(S_o_A_frags["sub_len"].mean()) + 1)
        self.ctx.set_insert_config(LIST_SIZE[:N_INSERT_BLOCKS], int(self.max_bounds_insert))
        self.ctx.upload_state(soa17_from_dict(S_o_A_frags, N))
        # CL:269-276
        self.np_init_prev = np.copy(S_o_A_frags["prev"])
        self.np_init_next = np.copy(S_o_A_frags["next"])
        self.np_init_orientable = np.array([np_sub_frags_id[S_o_A_frags["id_d"][i]]["w"] > 1 for i in range(N)],
                                           dtype=np.int32)
        self.np_init_ori = np.ones(N, dtype=np.int32)
        # the initial contig and position of every bin: what orientation_support's blocks are co-linear with (orientation_support.py)
        self.np_init_id_c = np.copy(S_o_A_frags["id_c"])
        self.np_init_pos = np.copy(S_o_A_frags["pos"])
        self.ctx.set_initial_genome(self.np_init_prev, self.np_init_next, self.np_init_orientable, self.id_frags_blacklisted)
        self.gpu_vect_frags = DeviceFrags(self.ctx)
        self.setup_distri_frags()
        self.param_simu = None
        self.param_simu_test = None
        self.likelihood_t = 0.0
        n, m, _ = self.ctx.renumber_contigs()
        self.n_contigs, self.mean_length_contigs = n, m
        self.candidates = []
        self.all_scores = np.zeros(0)
        # step_sampler leaves the 24 x C scores of its move in ``all_scores`` as the reference does (CL:1414-1431) -- which nothing
        # outside step_sampler ever reads (CL:1435-1454).  False (what ``simulation`` constructs: the reference's loop, IG:221-228):
        # ``all_scores`` stays None and the move is scored in two tiers, the exact kernel for the columns that can still win only.
        self.keep_all_scores = bool(keep_all_scores)

    # ------------------------------------------------------------ parameters
    def mean_kb(self):
        return np.float32(self.mean_len_bp_frags / 1000.0)  # CL:1120

    def setup_rippe_parameters(self, param, d_max):  # CL:2206-2221
        kuhn, lm, slope, d, fact = param
        fact = np.float32(np.abs(fact))
        kuhn = np.float32(np.abs(kuhn))
        lm = np.float32(np.abs(lm))
        c1 = np.float32((0.53 * np.power(lm / kuhn, slope)) * np.power(kuhn, -3))
        return np.array([(kuhn, lm, c1, np.float32(slope), np.float32(d), np.float32(d_max), np.float32(fact),
                          self.mean_value_trans)], dtype=PARAM_DTYPE)

    def set_param_simu(self, p, which=0):
        """p: dict or 1-element structured array (KA:91-100 fields)."""
        if isinstance(p, dict):
            arr = np.zeros(1, PARAM_DTYPE)
            for k in PARAM_NAMES:
                arr[k] = np.float32(p[k])
            p = arr
        p = np.array(p, dtype=PARAM_DTYPE).reshape(1)
        vals = [p[k][0] for k in PARAM_NAMES]
        if which == 0:
            self.param_simu = p
            self.ctx.set_params(vals, self.mean_kb(), 0)
            if self.param_simu_test is None:
                self.param_simu_test = p.copy()
                self.ctx.set_params(vals, self.mean_kb(), 1)
        else:
            self.param_simu_test = p
            self.ctx.set_params(vals, self.mean_kb(), 1)

    def estimate_parameters_rippe(self, max_dist_kb, size_bin_kb, display_graph=False):
        """CL:2239-2372: binned mean cis contacts of the first n_frags/10 sub-fragment rows, leastsq fit,
        cis/trans cut-off; then the initial likelihood."""
        if self.sparse_matrix is None:
            raise ValueError("estimate_parameters_rippe walks the rows of the input matrix, which a sampler built from coo= does not "
                             "keep: use estimate_parameters_from_genome (the law of the current genome, from the device)")
        self.bins = np.arange(size_bin_kb, max_dist_kb + size_bin_kb, size_bin_kb)
        self.bins_upd, self.mean_contacts_upd, p, self.y_estim, self.mean_value_trans, estim_max_dist = estimate_rippe_host(
            self.sparse_matrix, self.np_sub_frags_2_frags, self.S_o_A_frags, self.n_frags, self.mean_value_trans, max_dist_kb,
            size_bin_kb)
        self.set_param_simu(self.setup_rippe_parameters(p, estim_max_dist), 0)
        self.set_param_simu(self.param_simu, 1)
        self.eval_likelihood_init()

    # ------------------------------------------------------------- neighbours
    def setup_distri_frags(self):  # CL:3053-3101
        m = (self.sub_sampled_sparse_matrix + self.sub_sampled_sparse_matrix.T).tocsr()
        self.sym_sub_sampled_sparse_matrix = m
        self.distri_frags = {}
        fact = 3.0
        indptr, indices, data = m.indptr, m.indices, m.data
        for i in range(int(self.n_frags)):
            s, e = indptr[i], indptr[i + 1]
            yk, vk = indices[s:e], data[s:e]
            het = yk != i
            xk = yk[het]
            dat = np.float32(vk[het]) * fact
            if dat.sum() > 0:
                pk = dat / np.linalg.norm(dat, 1)
            else:
                tmp = np.ones_like(dat, dtype=np.float32)
                pk = tmp / tmp.sum()
            if len(xk) > 0:
                self.distri_frags[i] = dict(distri="ok", xk=np.array(xk), pk=pk)
            else:
                self.distri_frags[i] = dict(distri=None)
        # the same distributions as one CSR in the library's host memory: the draw of whole runs of moves happens there
        # (hip_lib.Neighbours / csrc/ig_draw.cpp), on numpy's generator state, off the interpreter
        n = int(self.n_frags)
        lens = np.array([len(self.distri_frags[i]["xk"]) if self.distri_frags[i]["distri"] is not None else 0 for i in range(n)],
                        dtype=np.int64)
        ok = [i for i in range(n) if lens[i]]
        nb_indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        nb_xk = np.concatenate([self.distri_frags[i]["xk"] for i in ok]).astype(np.int32) if ok else np.zeros(0, np.int32)
        nb_pk = np.concatenate([self.distri_frags[i]["pk"] for i in ok]).astype(np.float32) if ok else np.zeros(0, np.float32)
        self.neighbours = hip_lib.Neighbours(nb_indptr, nb_xk, nb_pk, n, self.id_frags_blacklisted)

    def return_neighbours(self, id_fA, delta0):  # CL:3103-3141
        ori_id = int(id_fA)  # id_d is the identity without repeats
        d = self.distri_frags[ori_id]
        if d["distri"] is not None:
            distri = d["pk"]
            n_max = min(delta0, np.nonzero(distri != 0)[0].shape[0])
            init_id = np.random.choice(d["xk"], n_max, p=distri, replace=False)
        else:
            init_id = np.random.choice(self.n_frags, delta0, replace=False)
        black = self.id_frags_blacklisted
        return [int(e) for e in init_id if e not in black]

    # ------------------------------------------------------------ likelihood
    def eval_likelihood_init(self):  # CL:1193-1243
        nz, z, _ = self.ctx.full_likelihood(0)
        self.curr_likelihood_on_nz = np.array([nz])
        # the reference's initial zero-pixel scalar is garbage (-inf): an int is passed where the kernel
        # takes a float (CL:743, quirk Q8).  It never reaches a score and likelihood_t is overwritten by
        # the first step_sampler (CL:1457); the well-defined value is reported instead.
        self.curr_likelihood_on_z = z
        self.likelihood_t = self.curr_likelihood_on_nz + z

    def eval_likelihood(self):  # CL:1245-1292
        nz, z, _ = self.ctx.full_likelihood(0)
        return nz

    def eval_likelihood_4_nuisance(self):  # CL:1296-1344: test parameters, coordinates of the state BEFORE the last move
        nz, z, _ = self.ctx.full_likelihood(1, use_prev_tables=True)
        self.curr_likelihood_nuis = np.array([nz]) + z
        return self.curr_likelihood_nuis

    # ------------------------------------------------------------------ moves
    def _clean(self, id_frag, candidates):
        c = sorted(int(x) for x in candidates)
        if int(id_frag) in c:
            # reachable only through the uniform fallback draw (CL:3124); the reference then scores
            # stale collector buffers (quirk Q13) -- no defined result to reproduce
            c = [x for x in c if x != int(id_frag)]
        return c

    def step_sampler(self, id_frag, n_neighbours, dt=None, candidates=None):  # CL:1401-1465
        # one library call (ig_step_draw): the draw of return_neighbours (CL:3103-3141) on numpy's generator state in place -- the same
        # list and the same state afterwards (tests/test_cpu_abi_and_host.py) -- the move, and the record as soon as it is complete
        res, sc, self.candidates = self.ctx.step_draw(self.neighbours, id_frag, max(1, int(n_neighbours)),
                                                      None if candidates is None else self._clean(id_frag, candidates), self.keep_all_scores)
        self.all_scores = sc
        self.o = res.o
        self.likelihood_t = res.o
        self.n_contigs = np.int32(res.n_contigs)
        self.mean_length_contigs = np.float32(res.mean_len)
        self.last_result = res
        return (res.o, res.dist, res.op_sampled, res.id_f_sampled, self.mean_length_contigs, self.n_contigs)

    def draw_candidates(self, frags, n_neighbours):
        """Candidates of consecutive moves, consuming numpy's global RNG exactly as successive
        step_sampler calls would (state-independent: CL:3103-3141)."""
        return self.neighbours.draw(frags, max(1, n_neighbours))

    def draw_candidates_python(self, frags, n_neighbours):
        """the same through return_neighbours, one numpy call per move (what draw_candidates is checked against)"""
        out = np.full((len(frags), max(1, n_neighbours)), -1, np.int32)
        for i, f in enumerate(frags):
            c = self._clean(f, self.return_neighbours(int(f), n_neighbours))
            out[i, : len(c)] = c
        return out

    def step_sampler_batch(self, frags, n_neighbours, candidates=None):
        """len(frags) consecutive step_sampler calls -- candidate draw included -- in ONE library call: a host thread draws
        the lists of the moves ahead on numpy's generator state while the launches of the moves in flight run; returns the
        structured result array (fields o, dist, op_sampled, id_f_sampled, mean_len, n_contigs, ...)."""
        frags = np.ascontiguousarray(frags, np.int32)
        if candidates is None:
            res, self.last_candidates = self.ctx.step_batch_draw(self.neighbours, frags, max(1, n_neighbours))
        else:
            res = self.ctx.step_batch(frags, candidates)
            self.last_candidates = candidates
        last = res[-1]
        self.o = self.likelihood_t = float(last["o"])
        self.n_contigs = np.int32(last["n_contigs"])
        self.mean_length_contigs = np.float32(last["mean_len"])
        return res

    def apply_replay_simu(self, id_fA, id_fB, op_sampled, dt=None):  # CL:2546-2553
        self.ctx.apply(int(id_fA), int(id_fB), int(op_sampled))
        self.gpu_vect_frags.copy_from_gpu()

    def test_copy_struct(self, id_fA, id_f_sampled, mode, max_id=None):  # CL:2094-2151
        self.ctx.apply(int(id_fA), int(id_f_sampled), int(mode))

    def modify_gl_cuda_buffer(self, id_fi=0, dt=None):  # CL:2715-2881
        n, m, max_id = self.ctx.renumber_contigs()
        self.n_contigs, self.mean_length_contigs = np.int32(n), m
        return np.int32(max_id)

    def bomb_the_genome(self):  # CL:1925-1948
        a = np.arange(0, self.n_new_frags, dtype=np.int32)
        np.random.shuffle(a)
        self.ctx.bomb(a)
        self.modify_gl_cuda_buffer(0, self.dt)

    def dist_inter_genome(self, tmp_gpu_vect_frags=None):  # CL:665-716
        return self.ctx.genome_distance()

    # -------------------------------------------------------------- nuisance
    def temperature(self, t, n_step):  # CL:3163-3165
        return 1.0

    def _sigmas(self, curr_param):  # CL:2970-2974
        kuhn, lm, c1, slope, d, d_max, fact, d_nuc = curr_param[0]
        self.sigma_fact = 10 ** (np.log10(fact) - 2)
        self.sigma_slope = 0.005
        self.sigma_d_max = 100
        self.sigma_d_nuc = 10 ** (np.log10(d_nuc) - 2)
        self.sigma_d = 10

    def _propose(self, curr_param, id_modif, normal):
        """the test parameters of one nuisance step (CL:2979-3017).  ``normal(sigma)`` -> the value numpy's
        ``np.random.normal(loc=0.0, scale=sigma)`` returns at this point of the stream (a Python float)."""
        kuhn, lm, c1, slope, d, d_max, fact, d_nuc = curr_param[0]
        if id_modif == 0:
            new_fact = fact + normal(self.sigma_fact)
            new_d_max = opti.estimate_max_dist_intra_nuis([kuhn, lm, slope, d, new_fact], d_nuc, d_max)
            c1 = np.float32((0.53 * np.power(lm / kuhn, slope)) * np.power(kuhn, -3))
            out = [(kuhn, lm, c1, slope, d, new_d_max, new_fact, d_nuc)]
        elif id_modif == 1:
            new_slope = slope + normal(self.sigma_slope)
            new_d_max = opti.estimate_max_dist_intra_nuis([kuhn, lm, new_slope, d, fact], d_nuc, d_max)
            c1 = np.float32((0.53 * np.power(lm / kuhn, new_slope)) * np.power(kuhn, -3))
            out = [(kuhn, lm, c1, new_slope, d, new_d_max, fact, d_nuc)]
        elif id_modif == 2:
            new_d_max = d_max + normal(self.sigma_d_max)
            new_d_nuc = opti.peval(new_d_max, [kuhn, lm, slope, d, fact])  # 5 values where 4 are read (quirk Q12)
            c1 = np.float32((0.53 * np.power(lm / kuhn, slope)) * np.power(kuhn, -3))
            out = [(kuhn, lm, c1, slope, d, new_d_max, fact, new_d_nuc)]
        else:
            if self.sigma_d_nuc <= 0:
                new_d_nuc = d_nuc
            else:
                new_d_nuc = d_nuc + normal(self.sigma_d_nuc)
            new_d_max = opti.estimate_max_dist_intra_nuis([kuhn, lm, slope, d, fact], new_d_nuc, d_max)
            c1 = np.float32((0.53 * np.power(lm / kuhn, slope)) * np.power(kuhn, -3))
            out = [(kuhn, lm, c1, slope, d, new_d_max, fact, new_d_nuc)]
        return np.array(out, dtype=PARAM_DTYPE)

    def _epoch8(self, curr_param):
        """what the proposals of the steps between two accepted ones share: the current parameters as eight float32 scalars, c1
        recomputed from them the way every branch of ``_propose`` recomputes it (CL:2985-3013)"""
        kuhn, lm, c1, slope, d, d_max, fact, d_nuc = curr_param[0]
        c1 = np.float32((0.53 * np.power(lm / kuhn, slope)) * np.power(kuhn, -3))
        return (kuhn, lm, c1, slope, d, d_max, fact, d_nuc)

    def _propose8(self, e8, id_modif, g):
        """``_propose`` on ``_epoch8``'s tuple with the standard normal ``g`` of the step, -> the eight float32 values of the
        structured array ``_propose`` builds (same expressions, same dtypes, same bits: tests/test_cpu_abi_and_host.py): the run loop
        computes one proposal per step on the host's critical path and needs the array only for the steps that are accepted"""
        kuhn, lm, c1, slope, d, d_max, fact, d_nuc = e8
        f32 = np.float32
        if id_modif == 0:
            new_fact = fact + (0.0 + float(self.sigma_fact) * g)
            new_d_max = opti.estimate_max_dist_intra_nuis([kuhn, lm, slope, d, new_fact], d_nuc, d_max)
            return (kuhn, lm, c1, slope, d, f32(new_d_max), f32(new_fact), d_nuc)
        if id_modif == 1:
            new_slope = slope + (0.0 + float(self.sigma_slope) * g)
            new_d_max = opti.estimate_max_dist_intra_nuis([kuhn, lm, new_slope, d, fact], d_nuc, d_max)
            c1 = f32((0.53 * np.power(lm / kuhn, new_slope)) * np.power(kuhn, -3))
            return (kuhn, lm, c1, f32(new_slope), d, f32(new_d_max), fact, d_nuc)
        if id_modif == 2:
            new_d_max = d_max + (0.0 + float(self.sigma_d_max) * g)
            new_d_nuc = opti.peval(new_d_max, [kuhn, lm, slope, d, fact])  # 5 values where 4 are read (quirk Q12)
            return (kuhn, lm, c1, slope, d, f32(new_d_max), fact, f32(new_d_nuc))
        new_d_nuc = d_nuc if self.sigma_d_nuc <= 0 else d_nuc + (0.0 + float(self.sigma_d_nuc) * g)
        new_d_max = opti.estimate_max_dist_intra_nuis([kuhn, lm, slope, d, fact], new_d_nuc, d_max)
        return (kuhn, lm, c1, slope, d, f32(new_d_max), fact, f32(new_d_nuc))

    def step_nuisance_parameters(self, dt, t, n_step):  # CL:2961-3051
        curr_param = np.copy(self.param_simu)
        self._sigmas(curr_param)
        id_modif = np.random.choice(4)
        out = self._propose(curr_param, id_modif, lambda sigma: np.random.normal(loc=0.0, scale=sigma))
        self.set_param_simu(out, 1)
        self.likelihood_nuis = self.eval_likelihood_4_nuisance()
        F_t = self.temperature(t, n_step)
        with np.errstate(over="ignore"):  # a much better likelihood at a low temperature: inf >= u, accepted
            ratio = np.exp((self.likelihood_nuis - self.likelihood_t) / F_t)
        u = np.random.rand()
        success = 0
        if ratio >= u:
            success = 1
            self.set_param_simu(out, 0)
            self.likelihood_t = self.likelihood_nuis
        kuhn, lm, c1, slope, d, d_max, fact, d_nuc = self.param_simu[0]
        y_rippe = opti.peval(self.bins, [kuhn, lm, slope, d, fact]) if hasattr(self, "bins") else None
        return (fact, d, d_max, d_nuc, slope, self.likelihood_t, success, y_rippe)

    def step_sampler_nuisance_batch(self, frags, n_neighbours, dt=None, t0=0, n_step=0):
        """``for f in frags: step_sampler(f, n, dt); step_nuisance_parameters(dt, t, n_step)`` -- the loop of
        instagraal.py:217-262 for cycles > 4 -- with the same results and the same generator stream, arranged for the GPU:

        * the stream of the whole run is drawn up front in the library (candidate lists, choice(4), the standard normal
          behind normal(0, sigma), the acceptance uniform: its consumption does not depend on the parameters);
        * the nuisance step's pass over all contacts reads the state BEFORE the move (quirk Q12) and only needs the move's
          score besides: it runs next to the move (``ig_nuis_step_begin`` / ``ig_nuis_end``);
        * a rejected step changes nothing a move reads: the moves are scored ahead in batches and decided one per step
          (``ig_nuis_run_begin``); an accepted step discards what was scored ahead;
        * while both run, the host prepares the next step's proposal (the root finding for d_max, CL:2983) for both
          outcomes of this one; the acceptance test itself and the first launches of the next step are one library call
          (``ig_nuis_step_next``), so that no Python runs between two steps' kernels.

        ``self.likelihood_nuis`` (the test likelihood of the last step: read nowhere outside the reference's method, CL:3023-3036) is
        set by the steps that go the plain way only -- a step rejected inside a chain is decided from an interval that
        lies below the threshold, and no value of it exists.

        -> (structured move results, list of the 8-tuples of step_nuisance_parameters with y_rippe = None)"""
        frags = np.ascontiguousarray(frags, np.int32)
        n = frags.size
        res = np.zeros(n, hip_lib.MOVE_RESULT_DTYPE)
        self._sigmas(np.copy(self.param_simu))
        # one step at a time: the one case where the stream depends on the parameters; an initial genome whose prev / next
        # links are not mutually inverse (the batch commit's bookkeeping needs that)
        if n == 0 or self.sigma_d_nuc <= 0 or not self.ctx.links_inverse():
            tuples = []
            for i, f in enumerate(frags):
                r = self.step_sampler(int(f), n_neighbours, dt)
                for k in res.dtype.names:
                    res[k][i] = getattr(self.last_result, k)
                tuples.append(self.step_nuisance_parameters(dt, t0 + i, n_step))
            return res, tuples
        with opti.quiet_runs():
            tuples, n_done = self._nuisance_run(frags, n_neighbours, t0, n_step, res)
        if n_done < n:
            # an accepted step took d_nuc to 0 (sigma_d_nuc with it: CL:2973): from the next step on the reference draws no normal for
            # id_modif == 3 (CL:3007-3010) and the stream drawn up front is not the reference's any more -- the rest one step at a time
            rest, more = self.step_sampler_nuisance_batch(frags[n_done:], n_neighbours, dt, t0 + n_done, n_step)
            res[n_done:] = rest
            tuples += more
        return res, tuples

    def _nuisance_run(self, frags, n_neighbours, t0, n_step, res):
        """the run of (move, nuisance step) pairs.  Two kinds of library calls: a CHAIN (``ig_nuis_chain_begin``: the pairs ahead as far
        as the device decides them alone -- moves from the batch's score records, steps rejected from the histogram tier's interval --
        while this loop prepares the proposals of the steps behind), and ONE pair the plain way for whatever a chain stops in front of
        (an accepted or undecided step, a conflict, a batch used up: ``ig_nuis_step_begin`` + ``ig_nuis_step_next``).  A rejected step
        changes no parameter, so the proposals of the steps ahead are a pure function of the current parameters and the pre-drawn
        stream: they are computed once per accepted step's epoch, ahead of their use."""
        import time as _t

        n = frags.size
        stream0 = np.random.get_state()  # (a run that ends early rewinds to its last step: `stop`)
        cands, id_modif, gauss, unif = self.neighbours.draw_nuisance(frags, max(1, n_neighbours))
        mean_kb = self.mean_kb()
        gauss_l, id_modif_l, unif_l = gauss.tolist(), id_modif.tolist(), unif.tolist()
        # (the base method returns 1.0: not called n times; one overridden in a subclass OR assigned on the instance is)
        plain_T = getattr(self.temperature, "__func__", None) is sampler.temperature
        temps = np.ones(n) if plain_T else np.array([float(self.temperature(t0 + i, n_step)) for i in range(n)])
        prof = self.nuis_profile = dict(propose=0.0, step=0.0, book=0.0, chain=0.0)
        trace = getattr(self, "nuis_step_trace", None)  # a list: (seconds, accepted) per plain step (tools/nuisance_rate.py)
        use_chain = hip_lib.nuis_chain_wanted()
        if not hasattr(self, "_nuis_acc_ema"):
            self._nuis_acc_ema = 0.0  # share of the recent steps that were accepted (kept from run to run)
        names = PARAM_NAMES
        curr = np.copy(self.param_simu)
        self._sigmas(curr)
        e8 = self._epoch8(curr)
        props = {}  # step -> the eight float32 test parameters of its proposal: valid while `curr` stands
        P = np.empty((n, 8), np.float32)  # ... and row i of it: a chain call hands over rows i .. i + K - 1 as they lie

        def prop(i):
            q = props.get(i)
            if q is None:
                q = props[i] = self._propose8(e8, id_modif_l[i], gauss_l[i])
                P[i] = q
            return q

        def as_array(p8):
            return np.array([p8], dtype=PARAM_DTYPE)

        last_test = [None]  # the test parameters of the last step that went the plain way

        # per step: the parameters it ends with (index into `epochs`), success; likelihood_t of an accepted step; the exact likelihood
        # of a step accepted ahead of its exact pass is filled in when the next plain step (or the end of the run) fetches it
        epochs = [self.param_simu]
        ep_of = np.zeros(n, np.int64)
        success_of = np.zeros(n, np.int8)
        lik_acc = {}
        patch = None  # (step, z)
        stop = [None]  # the run ends behind this many pairs: an accepted step left sigma_d_nuc <= 0 (step_sampler_nuisance_batch)

        def fill_in():
            j, zj = patch
            lik_acc[j] = np.array([self.ctx.nuis_exact_result()]) + zj

        def accepted(i, p8, lik_nuis, deferred, z):
            nonlocal curr, props, patch, e8
            out = as_array(p8)
            curr = np.copy(out)
            self.param_simu = out
            epochs.append(out)
            props = {}
            self._sigmas(curr)
            e8 = self._epoch8(curr)
            lik_acc[i] = lik_nuis
            if deferred:
                patch = (i, z)
            if self.sigma_d_nuc <= 0:
                stop[0] = i + 1

        def pairs_pipelined(i0, i1):
            """steps i0 .. i1 - 1, one pair per library call with the next step begun inside the call that ends this one (the loop of
            rounds 2 - 3: where chains are off, the histogram tier is not in use, or every third step is accepted -- a chain only ever
            rejects): while the GPU works on step i the proposal of step i + 1 for the case that this one is rejected is worked out;
            the one for the other case only if it comes to that"""
            nonlocal patch
            p8 = prop(i0)
            self.ctx.nuis_step_begin(i0, p8, mean_kb)
            for i in range(i0, i1):
                ta = _t.perf_counter()
                has_next = i + 1 < i1
                nxt = prop(i + 1) if has_next else None
                if patch is not None:  # (the exact pass of the step accepted last ran behind its decision: done by now)
                    fill_in()
                    patch = None
                t1 = _t.perf_counter()
                T = float(temps[i])
                r, nz, z, success = self.ctx.nuis_step_next(T, unif_l[i], nxt if has_next else None, None, mean_kb, has_next)
                t2 = _t.perf_counter()
                deferred = success == 3
                if deferred:
                    success = 1
                lik_nuis = np.array([nz]) + z
                began = success == 0  # (rejected: the library has begun step i + 1 with the parameters handed over)
                if success == 2:  # exp() within 1e-9 of u: the reference's own arithmetic decides
                    with np.errstate(over="ignore"):
                        ratio = np.exp((lik_nuis - r.o) / T)
                    success = 1 if ratio >= unif_l[i] else 0
                    if success:
                        self.ctx.nuis_accept()
                if success:
                    accepted(i, p8, lik_nuis, deferred, z)
                    has_next = has_next and stop[0] is None
                    nxt = prop(i + 1) if has_next else None  # (under the promoted parameters)
                ep_of[i] = len(epochs) - 1
                success_of[i] = success
                self.likelihood_nuis = lik_nuis
                last_test[0] = p8
                self._nuis_acc_ema = 0.9 * self._nuis_acc_ema + 0.1 * float(success)
                if has_next:
                    if not began:
                        self.ctx.nuis_step_begin(i + 1, nxt, mean_kb)
                    p8 = nxt
                t3 = _t.perf_counter()
                prof["propose"] += t1 - ta
                prof["step"] += t2 - t1
                prof["book"] += t3 - t2
                if trace is not None:
                    trace.append((t3 - ta, int(success)))
                if stop[0] is not None:
                    return

        self.ctx.nuis_run_begin(frags, cands)
        i = 0
        try_chain = False  # (the first pair scores the first batch: the plain way)
        empty = 0  # chains in a row that decided no pair (intervals that decide nothing: a void histogram tier, tests at the margin)
        LOOK = 2 * hip_lib.CHAIN_MAX
        _KCAP = 32  # sets of a chain call at most (16 / 24 / 32 / 40 / 48: 17.5 / 18.5 / 18.5 / 18.5 / 17.4 k pairs/s once the chain has settled)
        try:
            if not use_chain:
                pairs_pipelined(0, n)
                i = n
            while i < n and stop[0] is None:
                if self._nuis_acc_ema > 0.3 or empty >= 4:
                    # (the first steps of a run's first nuisance cycle: a third of the proposals accepted; or chains that get nowhere:
                    # a chain only ever rejects, and only from a certain interval -- one pair per call for a while, then another try)
                    i1 = min(n, i + (16 if empty < 4 else 32))
                    pairs_pipelined(i, i1)
                    i = i1
                    try_chain = False
                    empty = min(empty, 3)
                    continue
                if use_chain and try_chain:
                    ta = _t.perf_counter()
                    ready = 0  # proposals in hand from step i on
                    while ready < _KCAP and (i + ready) in props:
                        ready += 1
                    K = min(n - i, max(8, ready))
                    for t in range(i + ready, i + K):
                        prop(t)
                    self.ctx.nuis_chain_begin(i, P[i:i + K], unif[i:i + K], temps[i:i + K], mean_kb)
                    t = i + K
                    lim = min(n, i + K + LOOK)
                    while t < lim and not self.ctx.nuis_chain_done():  # the proposals of the steps behind, while the device works
                        if t not in props:
                            prop(t)
                        t += 1
                    j, reason = self.ctx.nuis_chain_end()
                    empty = 0 if j else empty + 1
                    self._nuis_acc_ema *= 0.9 ** j
                    ep_of[i:i + j] = len(epochs) - 1
                    i += j
                    prof["chain"] += _t.perf_counter() - ta
                    if reason == 0 and i < n:
                        continue  # every set was used: the next chain
                    if i >= n:
                        break
                    if reason == 6:  # the histogram tier is not in use: one pair per call from here on
                        pairs_pipelined(i, n)
                        i = n
                        break
                # ---- one pair the plain way
                ta = _t.perf_counter()
                p8 = prop(i)
                if patch is not None:  # (before the next step can be accepted ahead of its exact pass)
                    fill_in()
                    patch = None
                t1 = _t.perf_counter()
                T = float(temps[i])
                self.ctx.nuis_step_begin(i, p8, mean_kb)
                # (has_next without parameters: behind an accepted step the library re-scores the slots ahead under the promoted
                # parameters at once -- that needs nothing from here and runs while the proposals of the new epoch are worked out)
                r, nz, z, success = self.ctx.nuis_step_next(T, unif_l[i], None, None, mean_kb, i + 1 < n)
                t2 = _t.perf_counter()
                deferred = success == 3  # accepted from the screened interval: nz is its midpoint until the exact pass is through
                if deferred:
                    success = 1
                lik_nuis = np.array([nz]) + z
                rescored = success == 1
                if success == 2:  # exp() within 1e-9 of u: the reference's own arithmetic decides
                    with np.errstate(over="ignore"):
                        ratio = np.exp((lik_nuis - r.o) / T)
                    success = 1 if ratio >= unif_l[i] else 0
                    if success:
                        self.ctx.nuis_accept()
                if success:
                    accepted(i, p8, lik_nuis, deferred, z)
                ep_of[i] = len(epochs) - 1
                success_of[i] = success
                self.likelihood_nuis = lik_nuis
                last_test[0] = p8
                self._nuis_acc_ema = 0.9 * self._nuis_acc_ema + 0.1 * float(success)
                try_chain = rescored or not success  # (accepted by the arithmetic here: the slots ahead are void, a plain pair scores them)
                i += 1
                t3 = _t.perf_counter()
                prof["propose"] += t1 - ta
                prof["step"] += t2 - t1
                prof["book"] += t3 - t2
                if trace is not None:
                    trace.append((t3 - ta, int(success)))
        except BaseException:
            if patch is not None:
                try:  # (the run failed: whatever fetching the pending exact sum raises on the failed handle must not replace the cause)
                    fill_in()
                except Exception:
                    pass
            raise
        if patch is not None:
            fill_in()
        # the records of all moves at once; the 8-tuples from them
        n_done = n if stop[0] is None else stop[0]
        if n_done < n:  # the generator where the reference's is behind pair n_done - 1 (the same draws again: their number per pair is fixed while sigma_d_nuc > 0)
            np.random.set_state(stream0)
            self.neighbours.draw_nuisance(frags[:n_done], max(1, n_neighbours))
        res[:n_done] = self.ctx.batch_results(n_done)
        o_col = res["o"]
        tuples = []
        for k in range(n_done):
            kuhn, lm, c1, slope, d, d_max, fact, d_nuc = epochs[ep_of[k]][0]
            lik = lik_acc[k] if success_of[k] else o_col[k]
            tuples.append((fact, d, d_max, d_nuc, slope, lik, int(success_of[k]), None))
        self.param_simu = epochs[-1]
        if last_test[0] is not None:
            self.param_simu_test = as_array(last_test[0])
        self.likelihood_t = tuples[-1][5]
        last = res[n_done - 1]
        self.o = float(last["o"])
        self.n_contigs = np.int32(last["n_contigs"])
        self.mean_length_contigs = np.float32(last["mean_len"])
        self.candidates = [int(x) for x in cands[n_done - 1] if x >= 0]
        return tuples, n_done

    # ------------------------------------------------------------ contact map
    def contact_map(self, max_side=2048):
        """The contacts under the current genome as an exact integer image (``ig_contact_map``): the placed sub-fragments in the
        reference's ``full_order_high``, ``bin = max(1, ceil(T / max_side))`` of them per pixel -> (image int64 [side, side], bin).
        With ``max_side >= T`` it is the matrix the reference shows, ``(sparse_matrix + sparse_matrix.T)[order][:, order]``
        (CL:2598-2599), entry for entry.  The device holds the strict upper triangle only; the diagonal of the symmetrised input
        matrix is added here (a sampler built from ``coo=`` has none)."""
        image, b = self.ctx.contact_map(max_side)
        if self.sparse_matrix is not None and image.size:
            d = np.asarray(self.sparse_matrix.diagonal())
            nz = np.nonzero(d)[0]
            if nz.size:
                order = self.ctx.contact_map_order()
                where = np.full(d.size, -1, np.int64)
                where[order] = np.arange(order.size)
                nz = nz[where[nz] >= 0]
                px = where[nz] // b
                np.add.at(image, (px, px), d[nz].astype(np.int64))
        return image, b

    def display_current_matrix(self, filename, max_side=2048):  # CL:2555-2606
        """Writes the picture of the contact map of the current genome as the reference does (CL:2601-2605) and returns
        ``(full_order, dict_contig, full_order_high)``: the bins and, per contig id, its bins in genome order, and the sub-fragments
        in genome order (from the device).  Beyond ``max_side`` sub-fragments the picture is the binned image of ``contact_map``."""
        from . import contact_map as cmap

        g = self.gpu_vect_frags.copy_from_gpu()
        full_order, dict_contig, _ = cmap.genome_order(g.pos, g.id_c, g.activ, g.id_d, g.ori, self.np_sub_frags_id)
        full_order_high = self.ctx.contact_map_order().tolist()
        image, _ = self.contact_map(max_side)
        # matplotlib only here, and without pyplot: a figure on an Agg canvas of its own leaves the process's backend alone
        from matplotlib.backends.backend_agg import FigureCanvasAgg
        from matplotlib.figure import Figure

        fig = Figure(figsize=(14, 14))
        FigureCanvasAgg(fig)
        ax = fig.subplots()
        ax.imshow(image, vmax=np.percentile(image, 99) if image.size else None, interpolation="nearest")
        ax.axis("off")
        fig.savefig(filename, dpi=200, bbox_inches="tight")
        return full_order, dict_contig, full_order_high

    # ----------------------------------------------------------- distance law
    def distance_law(self, edges_kb=None):
        """The distance law P(s) of the current genome as the data shows it (``ig_distance_law``; the rule: ``distance_law.py``) next
        to the model curve the sampler is using.  ``edges_kb``: ascending bin edges in kb, default ``distance_law.default_edges``
        (geometric, from half a mean sub-fragment to beyond the longest contig).  -> the law's dict (edges, observed, pairs, the
        scalars) plus ``mean_per_pair`` (observed / pairs, nan where a bin holds no pair), ``centres_kb``, ``model`` (the Rippe curve
        under ``param_simu`` at the bin centres, the trans level beyond d_max: what a move is scored against; None without
        parameters) and ``mean_value_trans_observed`` (trans_observed / trans_pairs, nan without trans pairs).  No reference
        counterpart."""
        from . import distance_law as dlaw

        if edges_kb is None:
            d = self.ctx.debug_tables()[0]  # kb from the start of the contig: its maximum bounds every separation
            edges_kb = dlaw.default_edges(self.mean_kb(), float(d.max()) if d.size else 0.0)
        law = self.ctx.distance_law(dlaw.check_edges(edges_kb))
        law["mean_per_pair"] = dlaw.mean_per_pair(law)
        law["centres_kb"] = dlaw.bin_centres(law["edges"])
        law["model"] = None
        if self.param_simu is not None:
            kuhn, lm, c1, slope, d, d_max, fact, d_nuc = self.param_simu[0]
            with np.errstate(all="ignore"):
                y = np.asarray(opti.peval(law["centres_kb"], [kuhn, lm, slope, d, fact]), np.float64)
            law["model"] = np.where(law["centres_kb"] < d_max, y, np.float64(d_nuc))
        law["mean_value_trans_observed"] = law["trans_observed"] / law["trans_pairs"] if law["trans_pairs"] > 0 else float("nan")
        return law

    def display_distance_law(self, filename, edges_kb=None):
        """Writes a log-log plot of the observed per-pair means and of the model curve; returns what ``distance_law`` returns."""
        law = self.distance_law(edges_kb)
        # matplotlib only here, and without pyplot (as display_current_matrix)
        from matplotlib.backends.backend_agg import FigureCanvasAgg
        from matplotlib.figure import Figure

        fig = Figure(figsize=(8, 6))
        FigureCanvasAgg(fig)
        ax = fig.subplots()
        x, y = law["centres_kb"], law["mean_per_pair"]
        ok = np.isfinite(y) & (y > 0) & (x > 0)
        ax.loglog(x[ok], y[ok], "o", ms=3, label="observed contacts per pair")
        if law["model"] is not None:
            okm = (x > 0) & np.isfinite(law["model"]) & (law["model"] > 0)
            ax.loglog(x[okm], law["model"][okm], "-", label="model (param_simu)")
        if np.isfinite(law["mean_value_trans_observed"]) and law["mean_value_trans_observed"] > 0:
            ax.axhline(law["mean_value_trans_observed"], ls=":", color="grey", label="observed trans level")
        ax.set_xlabel("genomic separation s (kb)")
        ax.set_ylabel("contacts per sub-fragment pair")
        ax.legend()
        fig.savefig(filename, dpi=150, bbox_inches="tight")
        return law

    def estimate_parameters_from_genome(self, max_dist_kb, size_bin_kb):
        """``estimate_parameters_rippe`` on the law of the CURRENT genome instead of the first rows of the input matrix: works on a
        sampler built from ``coo=`` and at any point of a run.  Linear edges ``arange(0, max_dist_kb + size_bin_kb, size_bin_kb)``;
        the per-pair means of the bins that hold contacts, plus the trans level, at the bins' upper edges go through
        ``opti.estimate_param_rippe`` and ``opti.estimate_max_dist_intra`` the way ``estimate_rippe_host`` composes them (the trans
        level lowered tenfold before the cut-off is solved, CL:2338); then both parameter sets and the initial likelihood.  The
        trans level is the sampler's ``mean_value_trans``."""
        from . import distance_law as dlaw

        edges = np.arange(0, max_dist_kb + size_bin_kb, size_bin_kb).astype(np.float32)
        law = self.ctx.distance_law(dlaw.check_edges(edges))
        self.bins_upd, self.mean_contacts_upd, p, self.y_estim, self.mean_value_trans, estim_max_dist = fit_law(law, self.mean_value_trans)
        self.bins = np.array(law["edges"][1:], np.float64)
        self.set_param_simu(self.setup_rippe_parameters(p, estim_max_dist), 0)
        self.set_param_simu(self.param_simu, 1)
        self.eval_likelihood_init()
        return law

    # ------------------------------------------------------- junction profile
    def junction_profile(self, window=None, window_kb=None):
        """The junction support profile of the current genome (``ig_junction_profile``; the rule: ``junction_profile.py``): per
        junction between two neighbouring positions of the genome order the contacts that span it inside a window, the pairs that
        could, and what the model in use (``param_simu``) expects of them.  ``window``: in positions (default 64), or ``window_kb``:
        in kb, converted with the mean sub-fragment length.  -> the device's dict (window, n_placed, observed, pairs, expected_q,
        the scalars) plus ``expected`` (f64), ``ratio`` (observed / expected, nan where expected is 0), ``kind`` (per junction:
        ``junction_profile.KIND_*``), ``order`` (the sub-fragment at every position) and ``bins``: the table of the internal
        junctions at which the parent bin changes -- the joins the moves made or could break -- with the columns
        ``junction_profile.BIN_COLUMNS``.  No reference counterpart."""
        from . import junction_profile as jp

        if window is not None and window_kb is not None:
            raise ValueError("junction_profile: window or window_kb, not both")
        if window_kb is not None:
            window = jp.window_from_kb(window_kb, self.mean_kb())
        w = jp.check_window(jp.DEFAULT_WINDOW if window is None else window)
        prof = self.ctx.junction_profile(w)
        order = self.ctx.contact_map_order()
        _, _, stot, _, _ = self.ctx.debug_tables()
        parent = self.np_sub_frags_2_frags["x"].astype(np.int64)
        contig = self.gpu_vect_frags.copy_from_gpu().id_c.astype(np.int64)[parent]
        position = np.full(parent.size, -1, np.int64)
        position[order] = np.arange(order.size)
        prof["order"] = order
        prof["kind"] = jp.junction_kinds(stot, contig, position)
        prof["expected"] = jp.expected(prof)
        prof["ratio"] = jp.ratio(prof)
        prof["bins"] = jp.bin_table(prof, prof["kind"], parent[order], contig[order])
        return prof

    def weakest_junctions(self, n=20, min_pairs=None, window=None, window_kb=None, profile=None):
        """The ``n`` bin-level junctions (rows of ``junction_profile()["bins"]``) with the lowest observed / expected: where to look
        for a misjoin.  Only junctions whose window is at least half full count -- ``min_pairs`` defaults to half of
        w (w + 1) / 2 -- so that the ends of the contigs, which have few pairs, do not crowd the list."""
        from . import junction_profile as jp

        prof = self.junction_profile(window, window_kb) if profile is None else profile
        return jp.weakest(prof["bins"], n, jp.default_min_pairs(prof["window"]) if min_pairs is None else int(min_pairs))

    def display_junction_profile(self, filename, window=None, window_kb=None):
        """Writes a plot of observed / expected along the genome (log scale), the contig boundaries marked; returns what
        ``junction_profile`` returns."""
        from . import junction_profile as jp

        prof = self.junction_profile(window, window_kb)
        # matplotlib only here, and without pyplot (as display_current_matrix)
        from matplotlib.backends.backend_agg import FigureCanvasAgg
        from matplotlib.figure import Figure

        fig = Figure(figsize=(14, 5))
        FigureCanvasAgg(fig)
        ax = fig.subplots()
        y = np.where(prof["kind"] == jp.KIND_INTERNAL, prof["ratio"], np.nan)
        ok = np.isfinite(y) & (y > 0)
        x = np.arange(y.size)
        if ok.any():
            ax.semilogy(x[ok], y[ok], ".", ms=2, label="observed / expected (window of %d positions)" % prof["window"])
        edges = np.nonzero(prof["kind"] == jp.KIND_BOUNDARY)[0]
        for j in (edges if edges.size <= 2000 else edges[:0]):  # (beyond that the boundaries would be the picture)
            ax.axvline(j, color="grey", lw=0.3)
        ax.axhline(1.0, ls=":", color="black")
        ax.set_xlabel("position in the genome order (sub-fragments)")
        ax.set_ylabel("contacts across the junction: observed / expected")
        if ok.any():
            ax.legend()
        fig.savefig(filename, dpi=150, bbox_inches="tight")
        return prof

    # ------------------------------------------------------ assembly contacts
    def _assembly_contacts_frame(self, level, diagonal):
        """what the two methods below share: the device build, the order, the bins table, the diagonal per unit (or None)"""
        from . import assembly_contacts as ac

        ac.check_level(level)
        res = self.ctx.assembly_contacts(level)
        order = self.ctx.contact_map_order().astype(np.int64)
        parent = self.np_sub_frags_2_frags["x"].astype(np.int64)
        g = self.gpu_vect_frags.copy_from_gpu()
        table = ac.bins_table(order, parent, g.id_c, g.ori, self.S_o_A_sub_frags["len_bp"], level)
        diag, total = None, 0
        if diagonal and self.sparse_matrix is not None:
            d = np.asarray(self.sparse_matrix.diagonal()).astype(np.int64)
            unit = np.arange(order.size, dtype=np.int64) if level == "sub" else ac.units_along(parent[order])
            diag = np.zeros(res["n_units"], np.int64)
            np.add.at(diag, unit, d[order])
            total = int(diag.sum())
        return res, order, table, diag, total

    def assembly_contacts(self, level="sub", diagonal=True, balance=False):
        """The contacts in the coordinates of the current genome (``ig_assembly_contacts_build``; the rule: ``assembly_contacts.py``):
        every contact re-indexed to the units of the genome order -- ``level="sub"``: the positions of the contact map, ``"bin"``:
        the placed bins -- and sorted, as CSR arrays.  -> dict: ``rowptr`` (int64 [n_units + 1]), ``col`` (int32), ``count`` (int64),
        the scalars of ``assembly_contacts.SCALARS`` (they describe the device's result), ``order`` (the sub-fragment at every
        position), ``bins`` (``assembly_contacts.bins_table``: scaffold, start, end, parent bin, orientation per unit) and
        ``chrom_sizes`` ((contig ids, sizes)).  The device holds the strict upper triangle only: with ``diagonal=True`` and a
        sampler that has ``sparse_matrix`` (not one built from ``coo=``) the diagonal of the symmetrised input is merged in here as
        entries (u, u), first in their rows, as ``contact_map`` adds it to its image; their total is ``contacts_diagonal``.
        ``balance=True`` (or a dict of ``balance()``'s parameters): the dict gains ``weight`` (f64 per unit, ``balance(level)``) and
        ``balanced`` (count * weight[row] * weight[col] per entry; nan where a unit has no weight).
        The reference's counterpart, post.py, lifts the raw read pairs over instead: that is ``pairs_contacts``, which is not
        capped at sub-fragment resolution."""
        from . import assembly_contacts as ac

        res, order, table, diag, total = self._assembly_contacts_frame(level, diagonal)
        col, count = self.ctx.assembly_contacts_fetch(0, res["n_entries"])
        self.ctx.assembly_contacts_release()
        rowptr = res.pop("rowptr")
        if diag is not None:
            rowptr, col, count = ac.merge_diagonal(0, rowptr, col, count, diag)
        res.pop("n_entries")
        res.update(rowptr=rowptr, col=col, count=count, order=order, bins=table, chrom_sizes=ac.chrom_sizes(table), contacts_diagonal=total)
        if balance:
            from . import balance as bal

            res["weight"] = self.balance(level=level, **(balance if isinstance(balance, dict) else {}))["weight"]
            res["balanced"] = bal.balanced(count, ac.rows_of(rowptr), col, res["weight"])
        return res

    def write_assembly_contacts(self, folder, level="sub", diagonal=True, block_rows=None, balance=False):
        """Writes ``bins.bed``, ``pixels.tsv`` and ``chrom.sizes`` into ``folder``: what ``cooler load -f coo bins.bed pixels.tsv``
        takes.  The entries are fetched from the device and written by blocks of ``block_rows`` rows.  ``balance=True`` (or a dict
        of ``balance()``'s parameters): ``weights.tsv`` beside them -- unit, scaffold, start, end, weight per line of ``bins.bed``
        (``balance.write_weights``); the three other files are the same bytes.  -> the scalars (plus ``contacts_diagonal`` and
        ``pixels_written``)."""
        import os

        from . import assembly_contacts as ac

        res, _, table, diag, total = self._assembly_contacts_frame(level, diagonal)
        try:
            n = ac.write_all(folder, table, res["rowptr"], self.ctx.assembly_contacts_fetch, ac.DEFAULT_BLOCK_ROWS if block_rows is None else block_rows, diag)
        finally:
            self.ctx.assembly_contacts_release()
        out = {k: res[k] for k in ac.SCALARS}
        out.update(level=level, contacts_diagonal=total, pixels_written=n)
        if balance:
            from . import balance as bal

            bal.write_weights(os.path.join(folder, "weights.tsv"), table, self.balance(level=level, **(balance if isinstance(balance, dict) else {})))
        return out

    # ------------------------------------------------------------ zoom levels
    def _zoom_frame(self, diagonal):
        """the order, the sub-fragment table of the current genome and the self-contacts by position (or None)"""
        from . import assembly_contacts as ac

        order = self.ctx.contact_map_order().astype(np.int64)
        g = self.gpu_vect_frags.copy_from_gpu()
        table = ac.bins_table(order, self.np_sub_frags_2_frags["x"].astype(np.int64), g.id_c, g.ori, self.S_o_A_sub_frags["len_bp"], "sub")
        d = None
        if diagonal and self.sparse_matrix is not None:
            d = np.asarray(self.sparse_matrix.diagonal()).astype(np.int64)[order]
        return order, table, d

    @staticmethod
    def _zoom_units(table_sub, binsize, units):
        """-> (unit, U, the table of the units or None for a caller's own)"""
        from . import assembly_contacts as ac, zoom_levels as zl

        if (binsize is None) == (units is None):
            raise ValueError("zoom levels: give binsize (bp) or units (\"scaffold\", or (unit, n_units)), not both")
        if binsize is not None:
            unit, U = zl.units_of_positions(table_sub, binsize)
            return unit, U, zl.binnify(ac.chrom_sizes(table_sub), binsize)
        if isinstance(units, str):
            if units != "scaffold":
                raise ValueError("zoom levels: units is \"scaffold\" or (unit, n_units) (got %r)" % (units,))
            unit, U = zl.scaffold_units(table_sub)
            return unit, U, zl.scaffold_table(table_sub)
        unit, U = zl.check_units(units[0], units[1], table_sub.size)
        return unit, U, None

    @staticmethod
    def _diag_of_units(d, unit, U):
        if d is None:
            return None
        diag = np.zeros(U, np.int64)
        np.add.at(diag, unit, d)
        return diag

    def _balance_units(self, unit, n_units, ignore_diags=2, min_nnz=10, min_count=0, mad_max=0, tol=1e-5, max_iters=200):
        """``balance`` over a caller's units (``ig_balance_build_units``): the dict ``balance`` returns, level "units", without bins"""
        from . import balance as bal

        d = bal.check_ignore_diags(ignore_diags)
        tol, max_iters = bal.check_run(tol, max_iters)
        res = self.ctx.balance_build_units(unit, n_units, d)
        try:
            masked = bal.mask_units(res["nnz"], res["total"], min_nnz, min_count, mad_max)
            res.update(self.ctx.balance_run(np.where(masked, 0.0, 1.0), tol, max_iters))
        finally:
            self.ctx.balance_release()
        res["weight"], res["scale"] = bal.finish(res["b"], res["marg_final"], masked)
        res.update(masked=masked, ignore_diags=d, min_nnz=int(min_nnz), min_count=int(min_count), mad_max=mad_max, tol=tol, max_iters=max_iters)
        return res

    def resolution_contacts(self, binsize=None, units=None, diagonal=True, balance=False):
        """The contacts of the current genome at a fixed resolution (``ig_assembly_contacts_build_units``; the rule:
        ``zoom_levels.py``): ``binsize`` in bp -- a unit is a fixed bin of that many bp of a scaffold, the last one cut at the
        scaffold's end, and a sub-fragment counts for the bin that holds its midpoint --, or ``units="scaffold"`` (a unit is a
        scaffold), or a caller's ``(unit, n_units)`` per position.  -> the dict ``assembly_contacts`` returns, with ``bins`` the table of
        the fixed bins (contig, start, end; None for a caller's units), ``unit`` per position and ``units_without_position`` -- the
        fixed bins no midpoint falls into: above 0 the resolution is below what the fragments carry.  ``diagonal`` and ``balance`` as
        in ``assembly_contacts``; the ``balance`` dict may hold ``source`` and ``mode`` as in ``write_zoom_levels``.  The reference's post.py bins the raw read pairs instead: ``pairs_contacts(pairs, binsize)`` does that on the
        device, a pair counted where it falls."""
        from . import assembly_contacts as ac, balance as bal, zoom_levels as zl

        order, table_sub, d = self._zoom_frame(diagonal)
        unit, U, bins = self._zoom_units(table_sub, binsize, units)
        source, mode, bal_kw = self._balance_options(balance) if balance else ("contacts", "all", {})
        if mode != "all" and bins is None:
            raise ValueError("resolution_contacts: mode %r needs the scaffold of every unit, which a caller's units do not tell" % (mode,))
        if mode == "cis" and units == "scaffold":
            raise ValueError("resolution_contacts: mode \"cis\" keeps nothing of the scaffold matrix (every pixel off its diagonal lies between two scaffolds)")
        res = self.ctx.assembly_contacts_units(unit, U)
        try:
            col, count = self.ctx.assembly_contacts_fetch(0, res["n_entries"])
            if source == "snapshot":  # from the snapshot where it lies, before it goes
                weight = self._balance_snapshot(None if bins is None else bins["contig"], mode, **bal_kw)["weight"]
        finally:
            self.ctx.assembly_contacts_release()
        rowptr = res.pop("rowptr")
        res.pop("n_entries")
        diag = self._diag_of_units(d, unit, U)
        if diag is not None:
            rowptr, col, count = ac.merge_diagonal(0, rowptr, col, count, diag)
        res.update(rowptr=rowptr, col=col, count=count, order=order, bins=bins, unit=unit, chrom_sizes=ac.chrom_sizes(table_sub),
                   contacts_diagonal=0 if diag is None else int(diag.sum()), units_without_position=zl.units_without_position(unit, U),
                   binsize=None if binsize is None else int(binsize))
        if balance:
            res["weight"] = weight if source == "snapshot" else self._balance_units(unit, U, **bal_kw)["weight"]
            res["balanced"] = bal.balanced(count, ac.rows_of(rowptr), col, res["weight"])
        return res

    def scaffold_contacts(self, diagonal=True):
        """the scaffold by scaffold matrix of the current genome: ``resolution_contacts(units="scaffold")``"""
        return self.resolution_contacts(units="scaffold", diagonal=diagonal)

    def write_zoom_levels(self, folder, resolutions=_zoom_levels.DEFAULT_RESOLUTIONS, scaffolds=True, diagonal=True, balance=False, block_rows=None):
        """Writes the current genome's contacts at every bin size of ``resolutions`` (ascending, bp; the default:
        ``zoom_levels.DEFAULT_RESOLUTIONS``) to ``<folder>/resolutions/<bp>/{bins.bed, pixels.tsv, chrom.sizes}`` and (``scaffolds``) the
        scaffold matrix to ``<folder>/scaffolds/``, each what ``cooler load -f coo`` takes.  ``zoom_levels.plan`` decides how a level is
        made: built from the contacts, or -- its bin size a multiple of the level before it -- coarsened on the device from that
        level (``ig_assembly_contacts_coarsen``); the scaffold matrix is coarsened from the last level.  The bytes do not depend on the
        plan.  ``balance=True`` (or a dict of ``balance()``'s parameters): ``weights.tsv`` per level.  The dict may hold ``source`` --
        "contacts" (the default: every level's rows from a pass over the contacts, ``ig_balance_build_units``) or "snapshot" (from
        the level where it lies on the device, ``ig_balance_build_snapshot``: the same weights, and one more comment line in the file that
        names the source and the mode) -- and ``mode`` "cis" / "trans" (the
        pixels inside / between scaffolds only; they imply the snapshot; under "cis" the scaffold matrix has nothing to keep: no
        ``weights.tsv`` there and ``balanced: False`` in its dict).  -> a list, per level in order:
        dict of ``level`` (bp, or "scaffolds"), ``made`` (``("direct",)`` / ``("coarsen", factor)``), ``folder``, the scalars,
        ``n_units``, ``units_without_position``, ``contacts_diagonal`` and ``pixels_written``."""
        from . import assembly_contacts as ac, balance as bal, zoom_levels as zl

        import os

        source, mode, bal_kw = self._balance_options(balance) if balance else ("contacts", "all", {})
        res_list = zl.check_resolutions(resolutions)
        steps = list(zip(res_list, zl.plan(res_list)))
        order, table_sub, d = self._zoom_frame(diagonal)
        sizes = ac.chrom_sizes(table_sub)
        rows = ac.DEFAULT_BLOCK_ROWS if block_rows is None else block_rows
        out = []
        try:
            for i, (B, made) in enumerate(steps + ([("scaffolds", ("coarsen", "scaffolds"))] if scaffolds else [])):
                if B == "scaffolds":
                    (unit, U), bins, where = zl.scaffold_units(table_sub), zl.scaffold_table(table_sub), zl.scaffold_folder(folder)
                    res = self.ctx.assembly_contacts_coarsen(*zl.scaffold_map(sizes, res_list[-1]))
                else:
                    (unit, U), bins, where = zl.units_of_positions(table_sub, B), zl.binnify(sizes, B), zl.level_folder(folder, B)
                    if made[0] == "direct":
                        res = self.ctx.assembly_contacts_units(unit, U)
                    else:
                        res = self.ctx.assembly_contacts_coarsen(*zl.coarse_map(sizes, res_list[i - 1], made[1]))
                diag = self._diag_of_units(d, unit, U)
                n = zl.write_level(where, bins, res["rowptr"], self.ctx.assembly_contacts_fetch, rows, diag)
                one = {k: res[k] for k in ac.SCALARS}
                one.update(level=B, made=made, folder=where, units_without_position=zl.units_without_position(unit, U),
                           contacts_diagonal=0 if diag is None else int(diag.sum()), pixels_written=n)
                if balance and source == "snapshot":  # from the level where it lies on the device: built or coarsened a moment ago
                    one["balanced"] = not (B == "scaffolds" and mode == "cis")
                    if one["balanced"]:
                        bal.write_snapshot_weights(os.path.join(where, "weights.tsv"), bins, self._balance_snapshot(bins["contig"], mode, **bal_kw))
                elif balance:
                    w = self._balance_units(unit, U, **bal_kw)
                    w["level"] = "units"
                    bal.write_weights(os.path.join(where, "weights.tsv"), bins, w)
                out.append(one)
        finally:
            self.ctx.assembly_contacts_release()
        return out

    # ------------------------------------------------------- read pairs lifted
    contig_names = None  # {input contig name: id in S_o_A_sub_frags["id_c"]} (``simulation`` sets it): lets the pairs come by name
    # how the calls that take a pairs PATH read it (``_pairs_load``): "host" (``pairs_lift.read_pairs``, the Python line loop) or "device"
    # (the text parsed on the device and fed to the session without a round trip: ``pairs_text.py``).  An attribute and no keyword: the
    # parameter lists of ``pairs_contacts``, ``pairs_balance``, ``write_pairs_zoom_levels`` and ``pairs_distance_law`` are pinned
    pairs_reader = "host"

    def pairs_begin(self, reserve_pairs=0):
        """Opens a pairs session on the genome as it stands (``ig_pairs_begin``; the rule: ``pairs_lift.py``): the source table of
        ``pairs_lift.source_table`` goes to the device, the store of lifted pairs is empty.  A session open already is ended.  The
        session belongs to this genome: once a move or an edit has changed it the device REFUSES every further call of the session
        (``HipError``) until it is ended and begun again.  -> the table"""
        from . import assembly_contacts as ac, pairs_lift as pl

        self.pairs_end()
        sub = self.S_o_A_sub_frags
        order = self.ctx.contact_map_order().astype(np.int64)
        parent = self.np_sub_frags_2_frags["x"].astype(np.int64)
        g = self.gpu_vect_frags.copy_from_gpu()
        table = pl.source_table(sub["id_c"], sub["len_bp"], order, parent, g.id_c, g.ori, start_bp=sub["start_bp"] if "start_bp" in sub else None,
                                names=self.contig_names)
        table["table_sub"] = ac.bins_table(order, parent, g.id_c, g.ori, sub["len_bp"], "sub")
        table["table_bin"] = ac.bins_table(order, parent, g.id_c, g.ori, sub["len_bp"], "bin")
        self.ctx.pairs_begin(table, reserve_pairs)
        self._pairs = table
        return table

    def pairs_end(self):
        """ends the open pairs session, if there is one: the store and the table leave the device"""
        if getattr(self, "_pairs", None) is not None:
            self._pairs = None
            self.ctx.pairs_end()

    def lift_pairs(self, contig, pos1, contig2, pos2, strands=None):
        """Lifts read pairs from input-contig coordinates (``contig``, ``contig2``: ids as in ``S_o_A_sub_frags["id_c"]``, or names;
        1-based positions; ``strands``: ``pairs_lift.strand_codes`` or None) to the genome as it stands (``ig_pairs_lift``) -> the
        dict ``pairs_lift.lift_host`` returns: scaffold (its rank among the placed ones), 1-based position, position of the interval
        hit and reversed bit per end, the status code per pair, the scalars.  The kept pairs are appended to the store of the open
        session (one is opened if need be), from which ``pairs_contacts(None)`` and ``pairs_distance_law(None)`` are built."""
        from . import pairs_lift as pl

        if getattr(self, "_pairs", None) is None:
            self.pairs_begin()
        t = self._pairs
        return self.ctx.pairs_lift(pl.contig_ids(t, contig), pos1, pl.contig_ids(t, contig2), pos2, strands)

    def _pairs_fresh(self):
        """a session of its own for a call that brings its pairs: REFUSED while a session is open -- its store holds what the caller
        lifted, and is not thrown away behind their back (``pairs_end()`` first, or pass ``pairs=None`` to build from that store)"""
        if getattr(self, "_pairs", None) is not None:
            raise ValueError("pairs: a session is open and its store would be lost: pairs_end() first, or pass pairs=None to build from what it holds")
        return self.pairs_begin()

    def _pairs_load(self, pairs, chunk_pairs=None, reader=None):
        """``pairs``: None (the open session's store as it is), a path (a 4DN pairs file, read chunk by chunk) or arrays ``(contig,
        pos1, contig2, pos2[, strands])``: a fresh session with them lifted (refused while one is open: ``_pairs_fresh``) -> the summed
        scalars (plus ``malformed`` for a file).  ``reader``: how a file is read -- None: ``self.pairs_reader``; "host"
        (``pairs_lift.read_pairs``) or "device" (the text parsed on the device and fed to the session without a round trip:
        ``pairs_text.py``); the order in the store is unspecified either way"""
        from . import pairs_lift as pl

        reader = pl.check_reader(self.pairs_reader if reader is None else reader)
        if pairs is None:
            if getattr(self, "_pairs", None) is None:
                raise ValueError("pairs: no session is open (lift_pairs first, or give the pairs)")
            return {}
        t = self._pairs_fresh()
        total = dict.fromkeys(pl.SCALARS[:5], 0)
        try:
            if isinstance(pairs, (str, bytes)) or hasattr(pairs, "__fspath__"):
                if t["names"] is None:
                    raise ValueError("pairs: a pairs file names its contigs and this sampler has no contig_names")
                malformed = 0

                def add(res):
                    for k in total:
                        total[k] += res[k]

                if reader == "device":
                    malformed = pl.feed_device(pairs, t["names"], self.ctx, lambda: add(self.ctx.text_feed_pairs()),
                                               lambda c1, p1, c2, p2, strands: add(self.ctx.pairs_lift(c1, p1, c2, p2, strands, outputs=False)))
                else:
                    for ch in pl.read_pairs(pairs, t["names"], chunk_pairs or pl.DEFAULT_CHUNK_PAIRS):
                        malformed = ch["malformed"]
                        add(self.ctx.pairs_lift(ch["c1"], ch["p1"], ch["c2"], ch["p2"], ch["strands"], outputs=False))
                total["malformed"] = malformed
            else:
                res = self.ctx.pairs_lift(pl.contig_ids(t, pairs[0]), pairs[1], pl.contig_ids(t, pairs[2]), pairs[3], pairs[4] if len(pairs) > 4 else None, outputs=False)
                total.update((k, res[k]) for k in total)
        except BaseException:
            self.pairs_end()  # (the session was this call's own: a failed load leaves none)
            raise
        return total

    def _pairs_bins(self, kind, binsize):
        from . import assembly_contacts as ac, zoom_levels as zl

        t = self._pairs
        if kind == "sub":
            return t["table_sub"]
        if kind == "bin":
            return t["table_bin"]
        if kind == "scaffold":
            return zl.scaffold_table(t["table_sub"])
        return zl.binnify(ac.chrom_sizes(t["table_sub"]), binsize)

    def pairs_contacts(self, pairs, binsize=None, units=None, balance=False):
        """(How a pairs FILE is read, here and in ``pairs_balance``, ``write_pairs_zoom_levels``, ``pairs_distance_law`` and
        ``display_pairs_distance_law``: the attribute ``pairs_reader``, "host" or "device".)
        The map of read pairs at any resolution (``ig_pairs_pixels_build``): the pairs lifted onto the genome as it stands and
        counted per pixel -- ``binsize`` in bp (the bins of ``zoom_levels.binnify``; a pair counts where it falls), or ``units`` "sub"
        (the positions), "bin" (the placed bins: the rows of info_frags.txt) or "scaffold".  ``pairs``: a path or arrays -- lifted in a
        session of the call's own, ended behind it, and REFUSED (ValueError) while a session is open, whose store it would discard -- or
        None: the open session's store, which stays.  -> the dict ``resolution_contacts`` returns (rowptr, col, count, the scalars, ``bins``, ``chrom_sizes``,
        ``binsize``) plus the lift's scalars.  ``balance``: not offered by this method -- ``pairs_balance`` balances the same map from
        its snapshot on the device and returns this dict with the weights."""
        from . import assembly_contacts as ac, pairs_lift as pl

        if balance:
            raise NotImplementedError("pairs_contacts: balancing is pairs_balance's (the same map with its weights, balanced from the snapshot on the device)")
        if (binsize is None) == (units is None):
            raise ValueError("pairs: give binsize (bp) or units (\"sub\", \"bin\", \"scaffold\"), not both")
        lifted = self._pairs_load(pairs)
        try:
            kind, B, _, _ = pl.check_units(self._pairs, units if binsize is None else binsize)
            res = self.ctx.pairs_pixels(kind, B)
            try:
                col, count = self.ctx.assembly_contacts_fetch(0, res["n_entries"])
            finally:
                self.ctx.assembly_contacts_release()
            res.pop("n_entries")
            res.update(col=col, count=count, bins=self._pairs_bins(kind, B), chrom_sizes=ac.chrom_sizes(self._pairs["table_sub"]), binsize=B if kind == "binsize" else None,
                       units=kind)
            res.update(lifted)
        finally:
            if pairs is not None:
                self.pairs_end()
        return res

    def _balance_snapshot(self, group=None, mode="all", ignore_diags=2, min_nnz=10, min_count=0, mad_max=0, tol=1e-5, max_iters=200):
        """``balance`` over the snapshot that is on the device at this moment (``ig_balance_build_snapshot``; the rule:
        ``balance.balance_rows_host``), which stays there as it is: the dict ``_balance_units`` returns, with the scalars of
        ``balance.SNAPSHOT_SCALARS`` and ``mode``.  ``group``: the scaffold of every unit (read for "cis" / "trans")"""
        from . import balance as bal

        d = bal.check_ignore_diags(ignore_diags)
        tol, max_iters = bal.check_run(tol, max_iters)
        res = self.ctx.balance_build_snapshot(d, mode, group if bal.check_mode(mode) else None)
        try:
            masked = bal.mask_units(res["nnz"], res["total"], min_nnz, min_count, mad_max)
            res.update(self.ctx.balance_run(np.where(masked, 0.0, 1.0), tol, max_iters))
        finally:
            self.ctx.balance_release()
        res["weight"], res["scale"] = bal.finish(res["b"], res["marg_final"], masked)
        res.update(masked=masked, mode=mode, ignore_diags=d, min_nnz=int(min_nnz), min_count=int(min_count), mad_max=mad_max, tol=tol, max_iters=max_iters)
        return res

    @staticmethod
    def _balance_options(balance):
        """``balance`` of the writers (True, or a dict of ``balance()``'s parameters with ``source`` and ``mode``) -> (source, mode,
        the parameters); "cis" and "trans" imply the snapshot"""
        from . import balance as bal

        kw = dict(balance) if isinstance(balance, dict) else {}
        mode = kw.pop("mode", "all")
        source = kw.pop("source", "contacts" if bal.check_mode(mode) == 0 else "snapshot")
        if source not in ("contacts", "snapshot"):
            raise ValueError("balance: source is \"contacts\" or \"snapshot\" (got %r)" % (source,))
        if mode != "all" and source != "snapshot":
            raise ValueError("balance: mode %r is balanced from the snapshot (source=\"snapshot\")" % (mode,))
        return source, mode, kw

    def pairs_balance(self, pairs, binsize=None, units=None, mode="all", ignore_diags=2, min_nnz=10, min_count=0, mad_max=0, tol=1e-5, max_iters=200):
        """``pairs_contacts`` balanced (``ig_pairs_pixels_build``, then ``ig_balance_build_snapshot`` / ``ig_balance_run`` over the
        pixels where they lie on the device; the rule: ``balance.balance_rows_host``).  ``pairs``, ``binsize`` and ``units`` -- and the
        rules of the session -- as in ``pairs_contacts``; the parameters as in ``balance``; ``mode``: "all", or "cis" / "trans": only the
        pixels inside / between scaffolds are balanced (cooler's ``cis_only`` / ``trans_only``; "cis" at ``units="scaffold"`` has
        nothing to keep: ValueError; under "cis" the one mean of the iteration ties no two scaffolds' scales together: every
        scaffold's block comes out balanced, ``converged`` in general False -- DESIGN 4.29).  -> the dict ``pairs_contacts`` returns plus ``weight`` (f64 per unit, nan where it has none),
        ``balanced`` (count * weight[row] * weight[col] per entry), ``masked``, ``scale``, ``n_iters``, ``converged``, ``variance``,
        ``within_observed``, ``band_observed``, ``other_observed``, ``kept_observed``, ``entries``, and under ``balance_scalars`` all of
        ``balance.SNAPSHOT_SCALARS`` (``entries_in`` and ``entries_out`` mean the map's in this dict, the balancer's rows there)."""
        from . import assembly_contacts as ac, balance as bal, pairs_lift as pl

        bal.check_mode(mode)
        if (binsize is None) == (units is None):
            raise ValueError("pairs: give binsize (bp) or units (\"sub\", \"bin\", \"scaffold\"), not both")
        if mode == "cis" and units == "scaffold":
            raise ValueError("pairs_balance: mode \"cis\" keeps nothing of the scaffold matrix (every pixel off its diagonal lies between two scaffolds)")
        lifted = self._pairs_load(pairs)
        try:
            kind, B, _, _ = pl.check_units(self._pairs, units if binsize is None else binsize)
            res = self.ctx.pairs_pixels(kind, B)
            try:
                bins = self._pairs_bins(kind, B)
                w = self._balance_snapshot(bins["contig"], mode, ignore_diags, min_nnz, min_count, mad_max, tol, max_iters)
                col, count = self.ctx.assembly_contacts_fetch(0, res["n_entries"])
            finally:
                self.ctx.assembly_contacts_release()
            res.pop("n_entries")
            res.update(col=col, count=count, bins=bins, chrom_sizes=ac.chrom_sizes(self._pairs["table_sub"]), binsize=B if kind == "binsize" else None, units=kind)
            res.update(lifted)
            res.update((k, w[k]) for k in ("weight", "masked", "scale", "n_iters", "converged", "variance", "mode", "ignore_diags", "within_observed", "band_observed",
                                           "other_observed", "kept_observed", "entries"))
            res["balance_scalars"] = {k: w[k] for k in bal.SNAPSHOT_SCALARS}
            res["balanced"] = bal.balanced(count, ac.rows_of(res["rowptr"]), col, w["weight"])
        finally:
            if pairs is not None:
                self.pairs_end()
        return res

    def write_pairs_zoom_levels(self, folder, pairs, resolutions=_zoom_levels.DEFAULT_RESOLUTIONS, scaffolds=True, balance=False, block_rows=None):
        """``write_zoom_levels`` from read pairs: the same folders and writers, every level from the store of lifted pairs -- one
        build at the finest bin size of a run of multiples, coarsenings on the device behind it (``zoom_levels.plan``), the scaffold
        matrix coarsened from the last level.  ``balance=True`` (or a dict of ``pairs_balance``'s parameters, ``mode`` among them):
        ``weights.tsv`` per level (``balance.write_snapshot_weights``: its last line names the mode), every level balanced from the snapshot that is on the device at that
        moment -- built or coarsened --, the group of a fixed bin its scaffold; the other files are the same bytes.  Under ``mode="cis"``
        the scaffold matrix has nothing to keep: no ``weights.tsv`` there, and its dict says ``balanced: False``.  -> a list, per level:
        ``level``, ``made``, ``folder``, the scalars, ``pixels_written`` (and, balanced, ``balanced``, ``n_iters``, ``converged``)."""
        import os

        from . import assembly_contacts as ac, balance as bal, zoom_levels as zl

        if balance:
            source, mode, bal_kw = self._balance_options(balance)
            if "source" in (balance if isinstance(balance, dict) else {}) and source != "snapshot":
                raise ValueError("write_pairs_zoom_levels: a map of pairs is balanced from its snapshot (source=\"snapshot\")")
            bal.check_ignore_diags(bal_kw.get("ignore_diags", 2))
        res_list = zl.check_resolutions(resolutions)
        steps = list(zip(res_list, zl.plan(res_list)))
        rows = ac.DEFAULT_BLOCK_ROWS if block_rows is None else block_rows
        lifted = self._pairs_load(pairs)
        out = []
        try:
            sizes = ac.chrom_sizes(self._pairs["table_sub"])
            for i, (B, made) in enumerate(steps + ([("scaffolds", ("coarsen", "scaffolds"))] if scaffolds else [])):
                if B == "scaffolds":
                    bins, where = zl.scaffold_table(self._pairs["table_sub"]), zl.scaffold_folder(folder)
                    res = self.ctx.assembly_contacts_coarsen(*zl.scaffold_map(sizes, res_list[-1]))
                else:
                    bins, where = zl.binnify(sizes, B), zl.level_folder(folder, B)
                    if made[0] == "direct":
                        res = self.ctx.pairs_pixels("binsize", B)
                    else:
                        res = self.ctx.assembly_contacts_coarsen(*zl.coarse_map(sizes, res_list[i - 1], made[1]))
                n = zl.write_level(where, bins, res["rowptr"], self.ctx.assembly_contacts_fetch, rows)
                one = {k: res[k] for k in ac.SCALARS}
                one.update(level=B, made=made, folder=where, pixels_written=n)
                one.update(lifted)
                if balance:
                    one["balanced"] = not (B == "scaffolds" and mode == "cis")
                    if one["balanced"]:
                        w = self._balance_snapshot(bins["contig"], mode, **bal_kw)
                        bal.write_snapshot_weights(os.path.join(where, "weights.tsv"), bins, w)
                        one.update(n_iters=w["n_iters"], converged=w["converged"])
                out.append(one)
        finally:
            self.ctx.assembly_contacts_release()
            if pairs is not None:
                self.pairs_end()
        return out

    def pairs_distance_law(self, pairs, edges_bp=None, flip_strands=True):
        """P(s) of the read pairs on the genome as it stands, per strand combination (``ig_pairs_law``): the lifted pairs with both ends
        on one scaffold by |pos2 - pos1|.  ``edges_bp``: None for the distance law's default edges in bp.  ``flip_strands``: an end on
        a reversed bin has its strand flipped; False leaves the strands as read, as the reference does.  -> dict: ``counts`` (int64
        [4][n_edges - 1]: ++ +- -+ --), ``edges_bp``, ``norm_p`` (``pairs_lift.normalise``), pairs_stored / pairs_cis / pairs_trans and
        the lift's scalars."""
        from . import pairs_lift as pl

        lifted = self._pairs_load(pairs)
        try:
            if edges_bp is None:
                edges_bp = pl.default_edges_bp(self.mean_kb(), max(float(self._pairs["scaffold_len"].max(initial=0)) / 1000.0, 1.0))
            e = pl.check_edges(edges_bp)
            counts, sc = self.ctx.pairs_law(e, flip_strands)
        finally:
            if pairs is not None:
                self.pairs_end()
        out = dict(counts=counts, edges_bp=e, norm_p=pl.normalise(counts, e), flip_strands=bool(flip_strands))
        out.update(sc)
        out.update(lifted)
        return out

    def display_pairs_distance_law(self, filename, pairs, edges_bp=None, flip_strands=True):
        """``pairs_distance_law`` as a log-log plot, one curve per strand combination -> the law"""
        from matplotlib.backends.backend_agg import FigureCanvasAgg
        from matplotlib.figure import Figure

        from . import distance_law as dlaw, pairs_lift as pl

        law = self.pairs_distance_law(pairs, edges_bp, flip_strands)
        x = dlaw.bin_centres(law["edges_bp"])
        fig = Figure(figsize=(6, 4.5))
        FigureCanvasAgg(fig)
        ax = fig.subplots()
        for k, name in enumerate(pl.STRAND_COMBOS):
            y = law["norm_p"][k]
            ok = np.isfinite(y) & (y > 0) & (x > 0)
            if ok.any():
                ax.loglog(x[ok], y[ok], label=name)
        ax.set_xlabel("distance (bp)")
        ax.set_ylabel("P(s)")
        if ax.get_legend_handles_labels()[0]:
            ax.legend()
        fig.savefig(filename, dpi=150, bbox_inches="tight")
        return law

    def write_lifted_pairs(self, pairs_path, out_path, chunk_pairs=None, keep_session=False):
        """Rewrites a 4DN pairs file in the coordinates of the genome as it stands, gzip-compressed (``pairs_lift.write_lifted_pairs``:
        the header rewritten as the reference does, the kept pairs in input order), lifting on the device -> the scalars, ``malformed``
        and ``lines``.  The text is parsed and formatted on the host: that, not the lift, bounds this call -- so ``keep_session=True``
        leaves the session open with every kept pair (and its strands) in the store: ``pairs_contacts(None, ...)``,
        ``write_pairs_zoom_levels(folder, None, ...)`` and ``pairs_distance_law(None)`` then build from the one reading of the file
        (``pairs_end()`` behind them).  Refused while a session is open, as every call that brings its pairs."""
        from . import pairs_lift as pl

        t = self._pairs_fresh()
        done = False
        try:
            out = pl.write_lifted_pairs(pairs_path, out_path, t, lambda c1, p1, c2, p2, strands: self.ctx.pairs_lift(c1, p1, c2, p2, strands),
                                        chunk_pairs or pl.DEFAULT_CHUNK_PAIRS)
            done = True
            return out
        finally:
            if not (done and keep_session):
                self.pairs_end()

    # ---------------------------------------------------------------- balance
    def balance(self, level="bin", max_side=2048, ignore_diags=2, min_nnz=10, min_count=0, mad_max=0, tol=1e-5, max_iters=200):
        """The balancing weights of the current genome's contact map (``ig_balance_build`` / ``ig_balance_run``; the rule:
        ``balance.py``): one weight per unit -- ``level="sub"``: the positions of the genome order, ``"bin"``: the placed bins,
        ``"map"``: the pixels of ``contact_map(max_side)`` -- such that count * weight[u] * weight[v] has equal row sums (iterative
        correction, cooler's update).  Contacts inside a unit and closer than ``ignore_diags`` units are left out; a unit with fewer
        than ``min_nnz`` partners, fewer than ``min_count`` contacts or (``mad_max`` > 0) a coverage ``mad_max`` median absolute
        deviations below the median is masked (weight nan).  -> dict: ``weight``, ``b``, ``marg_final`` (f64 per unit), ``masked``,
        ``nnz``, ``total``, ``rowptr``, ``variance`` (f64 per iteration), ``n_iters``, ``converged``, ``scale``, the scalars of
        ``balance.SCALARS``, the parameters, ``order`` and ``bins`` (``assembly_contacts.bins_table``; None at level "map").  The rows and
        the iterations stay on the device; the mask is made here.  No reference counterpart."""
        from . import assembly_contacts as ac, balance as bal

        bal.check_level(level)
        d = bal.check_ignore_diags(ignore_diags)
        tol, max_iters = bal.check_run(tol, max_iters)
        res = self.ctx.balance_build(level, max_side, d)
        try:
            masked = bal.mask_units(res["nnz"], res["total"], min_nnz, min_count, mad_max)
            res.update(self.ctx.balance_run(np.where(masked, 0.0, 1.0), tol, max_iters))
        finally:
            self.ctx.balance_release()
        res["weight"], res["scale"] = bal.finish(res["b"], res["marg_final"], masked)
        res.update(masked=masked, level=level, max_side=int(max_side), ignore_diags=d, min_nnz=int(min_nnz), min_count=int(min_count), mad_max=mad_max, tol=tol,
                   max_iters=max_iters)
        order = self.ctx.contact_map_order().astype(np.int64)
        res["order"] = order
        res["bins"] = None
        if level != "map":
            g = self.gpu_vect_frags.copy_from_gpu()
            res["bins"] = ac.bins_table(order, self.np_sub_frags_2_frags["x"].astype(np.int64), g.id_c, g.ori, self.S_o_A_sub_frags["len_bp"], level)
        return res

    def balanced_map(self, max_side=2048, **kw):
        """``contact_map(max_side)`` balanced: the image as float64 times the outer product of the weights of its pixels
        (``balance(level="map", max_side=max_side, **kw)``); the rows and columns of masked pixels are nan -> (image f64 [side, side],
        bin)"""
        image, b = self.contact_map(max_side)
        w = self.balance(level="map", max_side=max_side, **kw)["weight"]
        return image.astype(np.float64) * np.outer(w, w), b

    def display_balanced_matrix(self, filename, max_side=2048, **kw):
        """Writes the picture of the balanced contact map of the current genome in the form of ``display_current_matrix`` (masked
        pixels stay blank) and returns ``(image, bin)`` of ``balanced_map``."""
        image, b = self.balanced_map(max_side, **kw)
        from matplotlib.backends.backend_agg import FigureCanvasAgg
        from matplotlib.figure import Figure

        fig = Figure(figsize=(14, 14))
        FigureCanvasAgg(fig)
        ax = fig.subplots()
        seen = image[np.isfinite(image)]
        ax.imshow(image, vmax=np.percentile(seen, 99) if seen.size else None, interpolation="nearest")
        ax.axis("off")
        fig.savefig(filename, dpi=200, bbox_inches="tight")
        return image, b

    # ----------------------------------------------------------- join support
    def join_support(self, window=None, window_kb=None):
        """Which scaffold ends the contacts would link (``ig_join_support_build``; the rule: ``join_support.py``): the junction
        profile for the joins the sampler did NOT make.  For every pair of ends of the placed linear contigs with at least one
        contact inside the window: the contacts that would span the join, the pairs that could, and what the model in use
        (``param_simu``) would expect of them with the two ends adjacent.  ``window``: in positions (default 64), or ``window_kb``.
        -> dict: ``rowptr`` (int64 [2 K + 1], CSR over the ends e = 2 k + side), ``col`` (int32), ``observed``, ``pairs``,
        ``expected_q`` (int64 per link), the scalars of ``join_support.SCALARS``, ``expected`` (f64), ``ratio`` (observed / expected,
        nan where expected is 0), ``ends`` (``join_support.ends_table``: scaffold, side, bin, sub-fragment, positions, bp per end),
        ``first_position`` / ``n_positions`` per contig and ``order``.  No reference counterpart."""
        from . import join_support as js

        if window is not None and window_kb is not None:
            raise ValueError("join_support: window or window_kb, not both")
        if window_kb is not None:
            window = js.window_from_kb(window_kb, self.mean_kb())
        w = js.check_window(js.DEFAULT_WINDOW if window is None else window)
        res = self.ctx.join_support(w)
        try:
            res["col"], res["observed"], res["pairs"], res["expected_q"] = self.ctx.join_support_fetch(0, res["n_links"])
        finally:
            self.ctx.join_support_release()
        order = self.ctx.contact_map_order().astype(np.int64)
        parent = self.np_sub_frags_2_frags["x"].astype(np.int64)
        g = self.gpu_vect_frags.copy_from_gpu()
        res["order"] = order
        res["ends"] = js.ends_table(res["first_position"], res["n_positions"], order, parent, g.id_c, self.S_o_A_sub_frags["len_bp"])
        res["expected"] = js.expected(res)
        res["ratio"] = js.ratio(res)
        return res

    def best_joins(self, n=20, min_pairs=None, window=None, window_kb=None, result=None):
        """The ``n`` links of ``join_support()`` with the highest observed / expected among those with at least ``min_pairs`` pairs
        (default: half a full window, as ``weakest_junctions``), each with the runner-up ratio of both of its ends
        (``join_support.best_joins``): a join is convincing when its ends have no close second."""
        from . import join_support as js

        res = self.join_support(window, window_kb) if result is None else result
        return js.best_joins(res, n, min_pairs)

    # ------------------------------------------------------ placement support
    def placement_support(self, window=None, window_kb=None, min_hosts=None):
        """Where the contacts say each bin belongs (``ig_placement_support``; the rule: ``placement_support.py``): every placed bin
        of a linear contig with the density of its contacts inside a window around where it sits (home) and around the densest
        other site of the genome (best) and the runner-up (second), the bin itself taken out of the order.  ``window``: in
        positions (default 64), or ``window_kb``; ``min_hosts``: the fewest positions a site's window must hold (default: the
        window).  -> dict: the per-bin arrays of ``placement_support.ARRAYS``, the scalars of ``placement_support.SCALARS``,
        ``home_density``, ``best_density`` (obs / (n_positions * hosts)), ``ratio`` = best / home (inf: nothing at home; nan:
        nothing anywhere), ``second_ratio`` (the runner-up's density over the best's), the sites for people -- ``scaffold``,
        ``best_scaffold``, ``second_scaffold`` (canonical ids: ``assembly_contacts.scaffold_names`` names them) and
        ``best_before`` / ``best_after`` / ``second_before`` / ``second_after``, the bins in front of and behind the site (-1:
        none) -- and ``order``.  No reference counterpart."""
        from . import placement_support as ps

        if window is not None and window_kb is not None:
            raise ValueError("placement_support: window or window_kb, not both")
        if window_kb is not None:
            window = ps.window_from_kb(window_kb, self.mean_kb())
        w = ps.check_window(ps.DEFAULT_WINDOW if window is None else window)
        res = self.ctx.placement_support(w, ps.check_min_hosts(min_hosts, w))
        order = self.ctx.contact_map_order().astype(np.int64)
        parent = self.np_sub_frags_2_frags["x"].astype(np.int64)
        res["order"] = order
        res.update(ps.densities(res))
        res.update(ps.sites_for_people(res, order, parent, self.gpu_vect_frags.copy_from_gpu().id_c))
        return res

    def misplaced_bins(self, n=20, min_ratio=1.0, result=None, window=None, window_kb=None, min_hosts=None):
        """The ``n`` bins of ``placement_support()`` whose contacts are denser somewhere else than at home by more than
        ``min_ratio``, best first (``placement_support.misplaced_bins``: inf first, ties by bin id)."""
        from . import placement_support as ps

        res = self.placement_support(window, window_kb, min_hosts) if result is None else result
        return ps.misplaced_bins(res, n, min_ratio)

    # ------------------------------------------------------ segment placement
    def segment_placement(self, level="block", segments=None, window=None, window_kb=None, min_hosts=None):
        """Where the contacts say a run of bins belongs, and which way round (``ig_segment_placement``; the rule:
        ``segment_placement.py``): placement support with a segment of the genome order for its guest -- a block carried along by
        an early wrong insertion is invisible bin by bin, its interior finds the rest of the block at home.  ``level``: "block", the
        maximal co-linear runs of bins of one initial contig (``orientation_support.block_segments``), "scaffold", one segment per
        linear placed scaffold, or "bin", one per placed bin (placement support's own answer); ``segments=(first, last)``: the
        caller's own intervals of positions, which override ``level``.  ``window``: in positions (default: placement support's,
        64), or ``window_kb``; ``min_hosts``: the fewest positions a site's window must hold (default: the window).  -> the rule's
        dict (the per-segment arrays of ``segment_placement.ARRAYS``, ``quadrants``, the scalars) plus ``level``, the densities
        (``home_density``, ``best_density``, ``ratio``, ``second_ratio``), the orientation at each site (``keep``, ``flip``,
        ``verdict``: [n_seg, 3] over home, best, second), the segments and sites for people (``first_bin``, ``last_bin``,
        ``scaffold``, ``best_scaffold``, ``best_before``, ``best_after`` and the same of ``second``), ``first_position`` and
        ``contig_positions`` per linear contig, and ``order``.  No reference counterpart."""
        from . import join_support as js, orientation_support as osup, segment_placement as sp

        if window is not None and window_kb is not None:
            raise ValueError("segment_placement: window or window_kb, not both")
        if window_kb is not None:
            window = sp.window_from_kb(window_kb, self.mean_kb())
        w = sp.check_window(sp.DEFAULT_WINDOW if window is None else window)
        try:
            mh = sp.check_min_hosts(min_hosts, w)
        except ValueError as e:
            raise ValueError(str(e).replace("placement support", sp.NAME)) from None
        order = self.ctx.contact_map_order().astype(np.int64)
        parent = self.np_sub_frags_2_frags["x"].astype(np.int64)
        g = self.gpu_vect_frags.copy_from_gpu()
        _, contig, stot, _, _ = self.ctx.debug_tables()
        position = np.full(parent.size, -1, np.int64)
        position[order] = np.arange(order.size)
        _, start, length, run = js.linear_runs(stot, contig, position)
        if segments is not None:
            first, last = (np.asarray(a) for a in segments)
            level = "custom"
        elif level == "bin":
            seg = osup.bin_segments(order, parent)
            first, last = seg["first"], seg["last"]
        elif level == "block":
            seg = osup.block_segments(order, parent, g.id_c, g.ori, g.id_d, self.np_init_id_c, self.np_init_pos)
            first, last = seg["first"], seg["last"]
        elif level == "scaffold":
            first, last = start.astype(np.int64), (start + length - 1).astype(np.int64)
        else:
            raise ValueError("segment_placement: level is 'block', 'scaffold' or 'bin' (got %r)" % (level,))
        res = self.ctx.segment_placement(w, first, last, mh)
        res["level"], res["order"] = level, order
        res["first_position"], res["contig_positions"] = start.astype(np.int32), length.astype(np.int32)
        res.update(sp.densities(res))
        res.update(sp.orientation_at(res))
        res.update(sp.sites_for_people(res, order, parent, g.id_c))
        return res

    def misplaced_segments(self, n=20, min_ratio=1.0, result=None, level="block", segments=None, window=None, window_kb=None, min_hosts=None):
        """The ``n`` segments of ``segment_placement()`` whose contacts are denser somewhere else than at home by more than
        ``min_ratio``, best first (``segment_placement.misplaced_segments``: inf first, ties by segment index)."""
        from . import segment_placement as sp

        res = self.segment_placement(level, segments, window, window_kb, min_hosts) if result is None else result
        return sp.misplaced_segments(res, n, min_ratio)

    # ---------------------------------------------------- orientation support
    def orientation_support(self, level="bin", segments=None, window=None, window_kb=None, model=True):
        """Which segments of the current genome the contacts would reverse (``ig_orientation_support``; the rule:
        ``orientation_support.py``): per segment the contacts between its two arms and the flanks on either side, in four quadrants,
        and what the model in use expects of the pairs that keep and that would flip it.  ``level``: "bin", one segment per placed
        bin, or "block", the maximal co-linear runs of bins of one initial contig (``orientation_support.block_segments``);
        ``segments=(first, last)``: the caller's own intervals of positions, which override ``level``.  ``window``: in positions
        (default 8), or ``window_kb``.  -> the device's dict (window, n_placed, n_seg, first, last, geometry, observed, expected_q,
        the scalars) plus ``level``, ``status``, the derived columns (``keep``, ``flip``, ``pairs``, ``ratio``, ``z`` and with the
        model ``expected_keep``, ``expected_flip``, ``llr``), the segments for people -- ``first_bin``, ``last_bin``, the bins at
        their ends, and ``scaffold`` (the canonical id: ``assembly_contacts.scaffold_names`` names it) -- and ``order``.  No
        reference counterpart."""
        from . import orientation_support as osup

        if window is not None and window_kb is not None:
            raise ValueError("orientation_support: window or window_kb, not both")
        if window_kb is not None:
            window = osup.window_from_kb(window_kb, self.mean_kb())
        w = osup.check_window(osup.DEFAULT_WINDOW if window is None else window)
        order = self.ctx.contact_map_order().astype(np.int64)
        parent = self.np_sub_frags_2_frags["x"].astype(np.int64)
        g = self.gpu_vect_frags.copy_from_gpu()
        if segments is not None:
            first, last = (np.asarray(a) for a in segments)
            level = "custom"
        elif level == "bin":
            seg = osup.bin_segments(order, parent)
            first, last = seg["first"], seg["last"]
        elif level == "block":
            seg = osup.block_segments(order, parent, g.id_c, g.ori, g.id_d, self.np_init_id_c, self.np_init_pos)
            first, last = seg["first"], seg["last"]
        else:
            raise ValueError("orientation_support: level is 'bin' or 'block' (got %r)" % (level,))
        res = self.ctx.orientation_support(w, first, last, model=model)
        res["level"], res["order"] = level, order
        res["status"] = res["geometry"][:, 0].copy()
        res.update(osup.derived(res))
        at = parent[order]
        res["first_bin"], res["last_bin"] = at[res["first"]], at[res["last"]]
        res["scaffold"] = g.id_c.astype(np.int64)[res["first_bin"]]
        return res

    def inverted_segments(self, n=20, min_observed=0, result=None, level="bin", segments=None, window=None, window_kb=None, model=True):
        """The ``n`` judged segments of ``orientation_support()`` with flip > keep, the most strongly reversed first
        (``orientation_support.inverted_segments``: by llr, by z without the model; ties by segment index)."""
        from . import orientation_support as osup

        res = self.orientation_support(level, segments, window, window_kb, model) if result is None else result
        return osup.inverted_segments(res, n, min_observed)

    # ------------------------------------------------------------ gap support
    def gap_support(self, level="block", junctions=None, gaps_kb=None, window=None, window_kb=None, model=True):
        """The distance the contacts put across each join of the current genome (``ig_gap_support``; the rule: ``gap_support.py``):
        per junction the contacts that span it, the pairs that could, and the two halves of a Poisson log-likelihood under every gap
        of a grid -- a true join across missing sequence still decays with distance, as P(s + g); a misjoin sits at the trans level.
        ``level``: "block", the junctions between two blocks of one scaffold (``gap_support.block_junctions``: the only places where
        a gap can exist), or "bin", every internal junction at which the bin changes; ``junctions``: the caller's own positions,
        which override ``level``.  ``gaps_kb``: the grid (default ``gap_support.default_gaps`` of the mean sub-fragment length and
        d_max); ``window``: in positions (default 64, at most 256), or ``window_kb``.  -> the device's dict (window, junction,
        gaps_kb, status, geometry, observed, pairs, log_q, expected_q, the scalars) plus ``level``, the junction table --
        ``scaffold`` (the canonical id: ``assembly_contacts.scaffold_names`` names it), ``left_bin``, ``right_bin`` --, ``order``,
        ``apart_q`` and, with the model, the columns of ``gap_support.derived`` (``ll``, ``ll_apart``, ``best``, ``gap_kb``,
        ``gap_lo``, ``gap_hi``, ``llr_gap``, ``llr_apart``, ``verdict``).  A level without a junction returns empty arrays (the device is
        not asked).  No reference counterpart."""
        from . import gap_support as gs
        from .hip_lib import model_values_host

        if window is not None and window_kb is not None:
            raise ValueError("gap_support: window or window_kb, not both")
        if window_kb is not None:
            window = min(gs.window_from_kb(window_kb, self.mean_kb()), gs.MAX_WINDOW)
        w = gs.check_window(gs.DEFAULT_WINDOW if window is None else window)
        if self.param_simu is None:
            raise ValueError("gap_support: set the parameters first (set_param_simu)")
        p8 = np.array([float(self.param_simu[k][0]) for k in PARAM_NAMES], np.float32)
        gaps = gs.default_gaps(self.mean_kb(), float(self.param_simu["d_max"][0])) if gaps_kb is None else gs.check_gaps(gaps_kb)
        order = self.ctx.contact_map_order().astype(np.int64)
        parent = self.np_sub_frags_2_frags["x"].astype(np.int64)
        g = self.gpu_vect_frags.copy_from_gpu()
        if junctions is not None:
            junc, level = np.asarray(junctions), "custom"
        elif level == "block":
            junc = gs.block_junctions(order, parent, g.id_c, g.ori, g.id_d, self.np_init_id_c, self.np_init_pos)["junction"]
        elif level == "bin":
            junc = gs.bin_junctions(order, parent, g.id_c)["junction"]
        else:
            raise ValueError("gap_support: level is 'block' or 'bin' (got %r)" % (level,))
        if junc.size:
            res = self.ctx.gap_support(w, junc, gaps, model=model)
        else:  # (fresh, a block is its contig: nothing to ask the device)
            K = int(gaps.size)
            res = dict(window=w, n_junctions=0, junction=np.zeros(0, np.int64), gaps_kb=gaps, status=np.zeros(0, np.int32), geometry=np.zeros((0, 4), np.int32),
                       observed=np.zeros(0, np.int64), pairs=np.zeros(0, np.int64), log_q=np.zeros((0, K), np.int64),
                       expected_q=np.zeros((0, K), np.int64) if model else None)
            res.update((k, 0) for k in gs.SCALARS)
        res["level"], res["order"] = level, order
        at = parent[order]
        res["left_bin"], res["right_bin"] = at[res["junction"] - 1], at[res["junction"]]
        res["scaffold"] = g.id_c.astype(np.int64)[res["right_bin"]]
        e_inf, l_inf = model_values_host(p8, np.array([np.inf], np.float32))
        res["apart_q"] = (int(e_inf[0]), int(l_inf[0]))
        if model:
            res.update(gs.derived(res))
        return res

    def gapped_joins(self, n=20, min_observed=0, result=None, level="block", junctions=None, gaps_kb=None, window=None, window_kb=None):
        """The ``n`` joins of ``gap_support()`` whose verdict is "gap" or "apart", the most decided first
        (``gap_support.gapped_joins``: by max(llr_gap, ll_apart - ll[0]), ties by junction)."""
        from . import gap_support as gs

        res = self.gap_support(level, junctions, gaps_kb, window, window_kb, True) if result is None else result
        return gs.gapped_joins(res, n, min_observed)

    # ---------------------------------------------------------- segment edits
    def score_rearrangements(self, edits, form="delta"):
        """The exact likelihood of the genome every segment edit would leave (``ig_edit_score``; the rule: ``rearrange.py``).
        ``edits``: int [n, 5] of (first_bin, last_bin, anchor, side, flip); ``form``: "delta" (one pass over the contacts per chunk of
        64 edits, the hot path) or "whole" (the from-scratch passes per edit, the definition) -- the same limbs.  -> a structured array
        (``rearrange.SCORE_DTYPE``): ``status``, ``nz``, ``z``, ``score`` = nz + z, ``delta`` against the current genome, ``limbs``.
        Nothing a move reads is changed.  No reference counterpart."""
        from . import rearrange as ra

        if form not in ra.FORMS:
            raise ValueError("score_rearrangements: form is 'delta' or 'whole' (got %r)" % (form,))
        e = ra.as_edits(edits)
        status, limbs, nz, z = self.ctx.edit_score(e, ra.FORMS.index(form))
        nz0, z0, _ = self.ctx.full_likelihood(0)
        out = np.zeros(e.shape[0], ra.SCORE_DTYPE)
        out["status"], out["nz"], out["z"], out["limbs"] = status, nz, z, limbs
        out["score"] = nz + z
        out["delta"] = out["score"] - (nz0 + z0)
        return out

    def apply_rearrangement(self, edit):
        """Commits one segment edit (``ig_edit_apply``) and refreshes ``likelihood_t``, ``n_contigs``, ``mean_length_contigs`` and
        ``gpu_vect_frags``.  -> the new likelihood; ValueError (nothing changed) for an edit the rule refuses."""
        status, limbs = self.ctx.edit_apply(edit)
        if status:
            raise ValueError("apply_rearrangement: the edit %s is refused with status %d (rearrange.check)" % (list(np.asarray(edit).ravel()), status))
        nz, z, now = self.ctx.full_likelihood(0)
        if not np.array_equal(now, limbs):
            raise RuntimeError("apply_rearrangement: the maintained sums behind the edit are %s, the from-scratch passes give %s" % (limbs.tolist(), now.tolist()))
        self.last_edit_limbs = limbs
        self.o = self.likelihood_t = nz + z
        n, m, _ = self.ctx.renumber_contigs()
        self.n_contigs, self.mean_length_contigs = np.int32(n), np.float32(m)
        self.gpu_vect_frags.copy_from_gpu()
        return self.likelihood_t

    def propose_rearrangements(self, n=20, window=None, orientation_window=None):
        """The edits the block-level reports propose on the current genome (``rearrange.propose``): the in-place flip of each of the
        ``n`` top ``inverted_segments`` (block level, window ``orientation_window``, default orientation support's), and for each of
        the ``n`` top ``misplaced_segments`` (block level, then scaffold level, window ``window``, default 64) every bin boundary of
        the best scaffold within the window of the best site, both ways round.  -> int32 [n_edits, 5]"""
        from . import rearrange as ra, segment_placement as sp

        w = sp.DEFAULT_WINDOW if window is None else int(window)
        inv = self.inverted_segments(n, level="block", window=orientation_window)
        mis = [self.misplaced_segments(n, level=level, window=w) for level in ("block", "scaffold")]
        return ra.propose(self.ctx.download_state(), inv, mis, n, w)

    def propose_cuts_joins(self, n=20, cuts=True, joins=True):
        """The edits of the ``n`` ``weakest_cuts`` and of the ``n`` ``strongest_joins`` of the current genome
        (``rearrange.propose_cuts_joins``) -> int32 [n_edits, 5]"""
        from . import rearrange as ra

        return ra.propose_cuts_joins(self.ctx.download_state(), self.cut_scores() if cuts else None, self.join_scores() if joins else None, n)

    # ---------------------------------------------------------- cut and join scores
    def cut_scores(self):
        """The likelihood change of EVERY cut of a linear contig, as far as it has a closed structure (``ig_cut_scores``; the rule:
        ``cut_join.py``): the cis contacts that span the junction become trans, the zero-pixel sum and the intra pair count of the two
        halves replace the contig's.  -> dict per bin f (the cut in front of it): ``valid``, ``contacts``, ``limbs`` (the delta limbs,
        exact integers in the units of ``score_rearrangements``), ``delta``.  What is left out (the contacts inside each half, whose
        f32 separation is rounded anew) is small: the scores rank, ``score_rearrangements`` decides.  No reference counterpart."""
        return self.ctx.cut_scores()

    def join_scores(self):
        """The same for EVERY link of two linear contigs with a contact between them, in its four orientations
        (``ig_join_scores_build``) -> dict: the linear contigs (``head_bin``, ``tail_bin``, ``n_sub``, ``length_bp``, numbered in
        ascending internal id), CSR ``rowptr`` / ``col`` over the pairs a < b, per pair ``contacts``, ``nz`` [4][2], ``z`` [2],
        ``dni``, ``delta`` [4] (link 2 sa + sb, side 0 the head, 1 the tail)."""
        return self.ctx.join_scores()

    def weakest_cuts(self, n=20, cuts=None):
        """the ``n`` cuts with the largest positive delta first -> ``cut_join.CUT_DTYPE`` rows, each with its edit"""
        from . import cut_join as cj

        return cj.weakest_cuts(self.ctx.download_state(), self.cut_scores() if cuts is None else cuts, n)

    def strongest_joins(self, n=20, joins=None):
        """the ``n`` links with the largest positive delta first, one row per link -> ``cut_join.LINK_DTYPE`` rows, each with its
        canonical edit"""
        from . import cut_join as cj

        return cj.strongest_joins(self.join_scores() if joins is None else joins, n)

    def polish(self, max_rounds=10, n=20, min_gain=0.0, window=None, orientation_window=None, cuts=False, joins=False):
        """Greedy polishing by segment edits: each round proposes (``propose_rearrangements``), scores every proposal exactly
        (``score_rearrangements``), takes the best edits on disjoint contigs (``rearrange.polish_round``) and applies them; it stops on
        a round with nothing to apply.  RuntimeError if the sums an apply returns differ from the limbs predicted for that edit (the
        first edit of a round exactly, the later ones by additivity).  Deterministic; draws nothing from numpy's generator.
        ``cuts`` / ``joins``: also propose the weakest cuts / the strongest joins (``cut_scores``, ``join_scores``); they are scored
        and checked like every other proposal.  -> the log: a list of dicts (round, edit, delta, likelihood after)."""
        from . import rearrange as ra

        log = []
        for rnd in range(int(max_rounds)):
            edits = self.propose_rearrangements(n, window, orientation_window)
            if cuts or joins:
                edits = np.concatenate([edits, self.propose_cuts_joins(n, cuts, joins)])
            if edits.shape[0] == 0:
                break
            scores = self.score_rearrangements(edits)
            take = ra.polish_round(scores, edits, self.ctx.download_state(), min_gain)
            if not take:
                break
            # the five limbs as three exact integers (value = hi * 2^32 + lo): the deltas of edits on disjoint contigs add
            exact = lambda l: ((int(l[0]) << 32) + int(l[1]), (int(l[2]) << 32) + int(l[3]), int(l[4]))  # noqa: E731
            base = exact(self.ctx.full_likelihood(0)[2])
            want = base
            for i in take:
                want = tuple(w + p - b for w, p, b in zip(want, exact(scores["limbs"][i]), base))
                like = self.apply_rearrangement(edits[i])
                if exact(self.last_edit_limbs) != want:
                    raise RuntimeError("polish: the sums behind edit %s are %s, predicted %s" % (edits[i].tolist(), exact(self.last_edit_limbs), want))
                log.append(dict(round=rnd, edit=edits[i].copy(), delta=float(scores["delta"][i]), likelihood=float(like)))
        return log

    # ----------------------------------------------------------- expected map
    def expected_map(self, max_side=2048):
        """What the model in use (``param_simu``) predicts for the pixels of ``contact_map(max_side)`` (``ig_expected_map``; the
        rule: ``expected_map.py``): one model value for every pair of sub-fragments that share a linear contig, summed per pixel
        on the device, the trans level for the pairs of different contigs.  -> the device's dict (side, bin, ``cis_q``,
        ``cis_pairs``, ``ring_pairs``, the scalars) plus ``total``, ``trans_pairs``, ``expected_q`` (int64 images) and ``expected``
        (f64: contacts).  Pixels that hold a pair on a ring get no model value for it (``ring_pairs`` says which).  No reference
        counterpart."""
        from . import expected_map as em

        if self.param_simu is None:
            raise ValueError("expected_map: set the parameters first (set_param_simu)")
        return em.compose(self.ctx.expected_map(max_side), em.quantize(np.float32(self.param_simu["v_inter"][0])))

    def residual_map(self, max_side=2048):
        """The observed image of the current genome (the device's: without the input matrix's diagonal, self-contacts have no model
        term) against ``expected_map``: -> dict: ``observed``, ``expected``, ``log2_ratio`` = log2(O / E), ``z`` = (O - E) / sqrt(E)
        (both nan where E == 0 or the pixel holds a ring pair: ``mask``), side, bin, n_placed, total."""
        from . import expected_map as em

        result = self.expected_map(max_side)
        observed, _ = self.ctx.contact_map(max_side)
        res = em.residuals(observed, result)
        res.update((k, result[k]) for k in em.SCALARS)
        return res

    def strongest_residuals(self, n=20, min_pairs=None, max_side=2048, residuals=None):
        """The ``n`` pixels off the diagonal with the largest z (``expected_map.strongest``): where a block has far more contacts
        with another than the model allows at their separation -- where it belongs.  ``min_pairs`` defaults to half of bin^2."""
        from . import expected_map as em

        res = self.residual_map(max_side) if residuals is None else residuals
        order = self.ctx.contact_map_order().astype(np.int64)
        parent = self.np_sub_frags_2_frags["x"].astype(np.int64)
        contig = self.gpu_vect_frags.copy_from_gpu().id_c.astype(np.int64)[parent]
        return em.strongest(res, n, min_pairs, contig[order])

    def display_residual_matrix(self, filename, max_side=2048):
        """Writes the picture of log2(observed / expected) of the current genome, clipped at +- 3, masked pixels grey; returns what
        ``residual_map`` returns."""
        from . import expected_map as em

        res = self.residual_map(max_side)
        # matplotlib only here, and without pyplot (as display_current_matrix)
        from matplotlib.backends.backend_agg import FigureCanvasAgg
        from matplotlib.figure import Figure

        fig = Figure(figsize=(14, 14))
        FigureCanvasAgg(fig)
        ax = fig.subplots()
        ax.set_facecolor("lightgrey")
        shown = np.ma.masked_invalid(np.clip(res["log2_ratio"], -em.CLIP_LOG2, em.CLIP_LOG2))
        im = ax.imshow(shown, cmap="RdBu_r", vmin=-em.CLIP_LOG2, vmax=em.CLIP_LOG2, interpolation="nearest")
        ax.set_xticks([])
        ax.set_yticks([])
        fig.colorbar(im, ax=ax, shrink=0.6, label="log2(observed / expected)")
        fig.savefig(filename, dpi=200, bbox_inches="tight")
        return res

    def free_gpu(self):  # CL:3167-3177
        self.ctx.close()
