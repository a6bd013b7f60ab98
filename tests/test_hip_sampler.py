"""GPU tests of the drop-in host surface (instagraal_amd.sampler.sampler) against the oracle run live:
larger problem, nuisance-parameter steps, batch == step-by-step, forced apply, error behaviour."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def make_pair(cfg, mode=1):
    from instagraal_amd import synth
    from instagraal_amd.sampler import sampler as hip_sampler
    from oracle import oracle_lib as ol
    from oracle.sampler_oracle import OracleSampler

    ol.build()
    prob = synth.make_problem(*synth.CONFIGS[cfg])
    kw = prob.sampler_kwargs()
    s = hip_sampler(**kw, device_id=0)
    s.set_param_simu(prob.params)
    s.bins = np.arange(1.0, 60.0, 1.0)
    s.eval_likelihood_init()
    o = OracleSampler(**kw, mode=ol.MODE_DET)
    o.set_param_simu(prob.params)
    o.bins = np.arange(1.0, 60.0, 1.0)
    o.eval_likelihood_init()
    return prob, s, o


def test_moves_with_large_counts_live_oracle():
    """contacts with counts >= 256 (beyond the LDS log-factorial table of the hot kernel) and >= 1024 (Stirling branch) in the
    slices of the moves: the fix-up path of k_score_list / k_delta / k_tail.  Scores bit-exact, same winners, same genome."""
    import copy

    import scipy.sparse as sp

    from instagraal_amd import synth
    from instagraal_amd.sampler import sampler as hip_sampler
    from oracle import oracle_lib as ol
    from oracle.sampler_oracle import OracleSampler

    ol.build()
    prob = copy.deepcopy(synth.make_problem(*synth.CONFIGS["tiny"]))
    cnt = prob.coo_cnt.copy()
    cnt[::5] *= 70
    cnt[::53] *= 500
    prob.coo_cnt = cnt
    M = prob.n_sub_frags
    prob.sub_csr = sp.csr_matrix((cnt, (prob.coo_row, prob.coo_col)), shape=(M, M), dtype=np.int32)
    prob.sub_csr.sort_indices()
    kw = prob.sampler_kwargs()
    s = hip_sampler(**kw, device_id=0)
    o = OracleSampler(**kw, mode=ol.MODE_DET)
    for x in (s, o):
        x.set_param_simu(prob.params)
        x.bins = np.arange(1.0, 60.0, 1.0)
        x.eval_likelihood_init()
    assert float(s.curr_likelihood_on_nz[0]) == float(o.gpu_curr_likelihood_nz[0])
    np.random.seed(5)
    frags = np.arange(prob.n_frags)
    np.random.shuffle(frags)
    for f in frags[:40]:
        cands = s.return_neighbours(int(f), 5)
        a = s.step_sampler(int(f), 5, candidates=cands)
        b = o.step_sampler(int(f), 5, o.dt, candidates=cands)
        assert np.array_equal(s.all_scores, o.all_scores)
        assert (a[0], a[1], a[2], a[3], float(a[4]), int(a[5])) == (b[0], b[1], b[2], b[3], float(b[4]), int(b[5]))
    assert np.array_equal(s.gpu_vect_frags.copy_from_gpu().soa17(), o.gpu_vect_frags.soa17())


def test_small_problem_live_oracle():
    """N=1000 / Z=150k, 40 moves with the reference's own candidate draw: scores bit-exact, same
    winner, same return tuple; final genome identical field by field."""
    prob, s, o = make_pair("small")
    assert float(s.curr_likelihood_on_nz[0]) == float(o.gpu_curr_likelihood_nz[0])
    np.random.seed(3)
    frags = np.arange(prob.n_frags)
    np.random.shuffle(frags)
    for f in frags[:40]:
        cands = s.return_neighbours(int(f), 5)
        a = s.step_sampler(int(f), 5, candidates=cands)
        b = o.step_sampler(int(f), 5, o.dt, candidates=cands)
        assert s.candidates == o.candidates
        assert np.array_equal(s.all_scores, o.all_scores)
        assert (a[0], a[1], a[2], a[3], float(a[4]), int(a[5])) == (b[0], b[1], b[2], b[3], float(b[4]), int(b[5]))
    assert np.array_equal(s.gpu_vect_frags.copy_from_gpu().soa17(), o.gpu_vect_frags.soa17())


def test_nuisance_trajectory_matches_golden():
    """step_sampler + step_nuisance_parameters (CL:2961-3051) against the reference-driven golden: RNG
    stream, fsolve'd d_max, the full-Z likelihood under test parameters on the PRE-move tables (Q12),
    accept/reject, and the parameter-dependent maintained sums after an accepted step."""
    from instagraal_amd import synth
    from instagraal_amd.sampler import sampler as hip_sampler

    g = np.load(os.path.join(GOLDEN, "tiny_nuis_mode1.npz"))
    prob = synth.make_problem(*synth.CONFIGS[str(g["config"])])
    np.random.seed(int(g["seed"]))
    s = hip_sampler(**prob.sampler_kwargs(), device_id=0)
    s.set_param_simu(prob.params)
    s.bins = np.arange(1.0, 60.0, 1.0)
    s.eval_likelihood_init()
    frags = np.arange(0, s.n_new_frags)
    np.random.shuffle(frags)
    nuis_from = int(g["nuis_from"])
    k = 0
    for t, f in enumerate(g["frag"]):
        r = s.step_sampler(int(f), 5, s.dt)
        c = list(s.candidates) + [-1] * (5 - len(s.candidates))
        assert c == list(g["cands"][t]), t
        exp = g["scores"][t][: len(s.candidates) * 24]
        assert np.array_equal(s.all_scores, exp), t
        assert [float(r[0]), float(r[1]), float(r[2]), float(r[3]), float(r[4]), float(r[5])] == list(g["ret"][t]), t
        if t >= nuis_from:
            q = s.step_nuisance_parameters(s.dt, t, len(g["frag"]))
            got = [float(q[0]), float(q[1]), float(q[2]), float(q[3]), float(q[4]), float(np.ravel(q[5])[0]), float(q[6])]
            assert got == list(g["nuis"][k]), (t, got, list(g["nuis"][k]))
            k += 1
    assert np.array_equal(np.random.get_state()[1][:8], g["rng_after"])
    assert np.array_equal(s.gpu_vect_frags.copy_from_gpu().soa17(), g["states"][-1])


def test_batch_equals_step_by_step():
    from instagraal_amd import synth
    from instagraal_amd.sampler import sampler as hip_sampler

    prob = synth.make_problem(*synth.CONFIGS["tiny"])
    outs = []
    for batch in (False, True):
        np.random.seed(5)
        s = hip_sampler(**prob.sampler_kwargs(), device_id=0)
        s.set_param_simu(prob.params)
        frags = np.arange(prob.n_frags)
        np.random.shuffle(frags)
        frags = frags[:50]
        if batch:
            res = s.step_sampler_batch(frags, 5)
            rows = [(float(r["o"]), float(r["dist"]), int(r["op_sampled"]), int(r["id_f_sampled"]), float(r["mean_len"]),
                     int(r["n_contigs"])) for r in res]
        else:
            rows = []
            for f in frags:
                r = s.step_sampler(int(f), 5)
                rows.append((float(r[0]), float(r[1]), int(r[2]), int(r[3]), float(r[4]), int(r[5])))
        outs.append((rows, s.gpu_vect_frags.copy_from_gpu().soa17(), np.random.get_state()[1][:4].copy()))
    assert outs[0][0] == outs[1][0]
    assert np.array_equal(outs[0][1], outs[1][1])
    assert np.array_equal(outs[0][2], outs[1][2])


@pytest.mark.parametrize("cfg,n_moves", [("tiny", 150), ("small", 400)])
def test_speculative_batches_equal_one_move_at_a_time(cfg, n_moves):
    """ig_step_batch scores W moves against one state and commits them in order on the device -- as fresh batches (rounds 1 - 4) or over
    a window of slots that stay scored from launch to launch (round 5); every result record, the final genome, the
    maintained exact sums and the pre-move tables (quirk Q12) must not depend on the rule or its width."""
    from instagraal_amd import hip_lib, synth
    from instagraal_amd.sampler import sampler as hip_sampler

    prob = synth.make_problem(*synth.CONFIGS[cfg])
    outs = []
    try:
        # one move at a time; round 4's batches (no window) of 2 .. 32 slots; round 5's window of scored slots, 2 .. 64 wide (kept slots
        # validated on the device against the live genome: IG_WINDOW_CHECK)
        os.environ["IG_WINDOW_CHECK"] = "1"
        modes = [(1, 0), (2, 0), (5, 0), (16, 0), (32, 0), (24, 2), (24, 7), (24, 48), (24, 64)]
        for W, win in modes:
            hip_lib.set_batch_width(W)
            hip_lib.set_window(win)
            np.random.seed(9)
            s = hip_sampler(**prob.sampler_kwargs(), device_id=0)
            s.set_param_simu(prob.params)
            s.eval_likelihood_init()
            frags = np.resize(np.random.permutation(prob.n_frags), n_moves).astype(np.int32)
            cands = s.draw_candidates(frags, 5)
            res = s.ctx.step_batch(frags, cands)
            sums, ints = s.ctx.debug_globals()
            _, _, limbs = s.ctx.full_likelihood(0)
            assert (int(sums[0]), int(sums[1])) == (int(limbs[0]), int(limbs[1])), W
            prev = s.ctx.full_likelihood(0, use_prev_tables=True)
            outs.append((res.tobytes(), s.gpu_vect_frags.copy_from_gpu().soa17(), [int(x) for x in sums], int(ints[0]),
                         [int(x) for x in prev[2]], [int(x) for x in s.ctx.valid_insert()], s.ctx.batch_stats()))
    finally:
        hip_lib.set_batch_width(24)
        hip_lib.set_window(48)
        os.environ.pop("IG_WINDOW_CHECK", None)
    for W, o in zip(modes[1:], outs[1:]):
        assert o[0] == outs[0][0], W
        assert np.array_equal(o[1], outs[0][1]), W
        assert o[2:6] == outs[0][2:6], W
    assert outs[3][6]["batches"] < n_moves  # speculation actually happened
    assert outs[7][6]["batches"] < outs[3][6]["batches"]  # ... and a window of 48 needs fewer launch chains than batches of 16


@pytest.mark.parametrize("cfg,n_moves", [("tiny", 200), ("small", 300), ("bigctg", 60)])
def test_step_draw_equals_step(cfg, n_moves):
    """``step_sampler`` goes through ig_step_draw (round 5: the draw inside the call, lists and results through mapped host memory,
    the move scored and committed as a batch of one by the fused commit kernel): every 6-tuple, every score of all_scores
    (CL:1414-1431), the candidate lists, numpy's generator state and the final genome must be those of ig_step's way (the one-move
    kernels: IG_STEP_DRAW_FAST=0) -- with the draw inside the call and with the caller's candidates; bigctg: windowed winners, which
    the one-move tail finishes.  A third run without all_scores (``keep_all_scores=False``: the batch of one scored in two tiers)."""
    from instagraal_amd import synth
    from instagraal_amd.sampler import sampler as hip_sampler

    prob = synth.make_problem(*synth.CONFIGS[cfg])
    outs = []
    try:
        for fast, keep in ((0, True), (1, True), (1, False)):
            os.environ["IG_STEP_DRAW_FAST"] = str(fast)
            np.random.seed(21)
            s = hip_sampler(**prob.sampler_kwargs(), device_id=0, keep_all_scores=keep)
            s.set_param_simu(prob.params)
            s.eval_likelihood_init()
            frags = np.resize(np.random.permutation(prob.n_frags), n_moves)
            rows, scores, cands = [], [], []
            for i, f in enumerate(frags):
                if i % 3 == 2:  # the caller's own list (the reference's way to the same draw)
                    a = s.step_sampler(int(f), 5, candidates=s.return_neighbours(int(f), 5))
                else:
                    a = s.step_sampler(int(f), 5)
                rows.append((a[0], a[1], int(a[2]), int(a[3]), float(a[4]), int(a[5])))
                scores.append(np.array(s.all_scores) if keep else s.all_scores)
                cands.append(list(s.candidates))
            st = np.random.get_state()
            outs.append((rows, scores, cands, st[1].tobytes(), st[2], s.gpu_vect_frags.copy_from_gpu().soa17(),
                         [int(x) for x in s.ctx.valid_insert()], s.ctx.debug_step_stats(), s.ctx.debug_screen_stats()))
            s.free_gpu()
    finally:
        os.environ.pop("IG_STEP_DRAW_FAST", None)
    a, b, c = outs
    assert a[0] == b[0] == c[0]
    assert all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))
    assert all(x is None for x in c[1])  # keep_all_scores=False (what ``simulation`` constructs): no scores, two-tier scoring
    assert a[2] == b[2] == c[2] and a[3] == b[3] == c[3] and a[4] == b[4] == c[4]
    assert np.array_equal(a[5], b[5]) and np.array_equal(a[5], c[5]) and a[6] == b[6] == c[6]
    assert a[7]["calls"] == 0 and b[7]["calls"] >= n_moves and c[7]["calls"] >= n_moves
    assert b[8][2] == 0 and c[8][2] > 5 * c[8][3] > 0, (b[8], c[8])  # columns screened / scored exactly: the second tier is a small share
    if cfg == "bigctg":
        assert b[7]["tails"] > 0 and c[7]["tails"] > 0  # windowed winners that change the genome: finished by the one-move tail


def test_large_windows_match_oracle():
    """Contigs of thousands of sub-fragments: the 32 KB column stage of k_score_list<4096> and, above 4096 sub-fragments,
    the unstaged path (8-byte gathers from L2), against the oracle move by move; then a batch."""
    prob, s, o = make_pair("bigctg")
    soa = prob.sampler_kwargs()["S_o_A_frags"]
    assert soa["sub_l_cont"].max() > 4096 and np.sum((soa["sub_l_cont"] > 1024) & (soa["sub_l_cont"] <= 4096)) > 0
    np.random.seed(4)
    frags = np.random.permutation(prob.n_frags)[:24]
    for f in frags[:6]:
        cands = s.return_neighbours(int(f), 5)
        a = s.step_sampler(int(f), 5, candidates=cands)
        b = o.step_sampler(int(f), 5, o.dt, candidates=cands)
        assert np.array_equal(s.all_scores, o.all_scores)
        assert (a[0], a[1], a[2], a[3], int(a[5])) == (b[0], b[1], b[2], b[3], int(b[5]))
    rest = frags[6:].astype(np.int32)
    cands = s.draw_candidates(rest, 5)
    res = s.ctx.step_batch(rest, cands)
    for f, c, r in zip(rest, cands, res):
        b = o.step_sampler(int(f), 5, o.dt, candidates=[int(x) for x in c if x >= 0])
        assert (float(r["o"]), float(r["dist"]), int(r["op_sampled"]), int(r["id_f_sampled"])) == (b[0], b[1], b[2], b[3])
    assert np.array_equal(s.gpu_vect_frags.copy_from_gpu().soa17(), o.gpu_vect_frags.soa17())


def test_checked_scoring_path_equals_the_hot_one(monkeypatch):
    """IG_ABLATE=2 sends every column of k_score_list through the out-of-line checked loop (the one windows with a circular
    contig or parameters outside the one-log domain take): result records, genome and exact sums identical to the hot loop"""
    from instagraal_amd import synth
    from instagraal_amd.sampler import sampler as hip_sampler

    prob = synth.make_problem(*synth.CONFIGS["small"])
    runs = []
    for abl in ("0", "2"):
        monkeypatch.setenv("IG_ABLATE", abl)
        s = hip_sampler(**prob.sampler_kwargs(), device_id=0)
        s.set_param_simu(prob.params)
        s.eval_likelihood_init()
        np.random.seed(9)
        frags = np.random.permutation(prob.n_frags)[:60].astype(np.int32)
        res = s.ctx.step_batch(frags, s.draw_candidates(frags, 5))
        runs.append((res.tobytes(), s.gpu_vect_frags.copy_from_gpu().soa17().tobytes(), [int(x) for x in s.ctx.full_likelihood(0)[2][:2]]))
        s.free_gpu()
    assert runs[0] == runs[1]


def test_batch_outcome_by_copy_equals_polled_flag(monkeypatch):
    """IG_NO_HOST_FLAG=1: the host learns a batch's outcome by copy + synchronise instead of polling the mapped host copy
    k_decide_batch writes; same result records, same genome"""
    from instagraal_amd import synth
    from instagraal_amd.sampler import sampler as hip_sampler

    prob = synth.make_problem(*synth.CONFIGS["small"])
    runs = []
    for flag in ("0", "1"):
        monkeypatch.setenv("IG_NO_HOST_FLAG", flag)
        s = hip_sampler(**prob.sampler_kwargs(), device_id=0)
        s.set_param_simu(prob.params)
        s.eval_likelihood_init()
        np.random.seed(11)
        frags = np.random.permutation(prob.n_frags)[:80].astype(np.int32)
        res = s.ctx.step_batch(frags, s.draw_candidates(frags, 5))
        runs.append((res.tobytes(), s.gpu_vect_frags.copy_from_gpu().soa17().tobytes()))
        s.free_gpu()
    assert runs[0] == runs[1]


def test_slice_pool_overflow_reruns_the_slot(monkeypatch):
    """a pool that holds one move's slice lists but not a batch's: the slots that do not fit are flagged by k_offsets and
    re-run at the head of the next batch; a pool that does not even hold the first move of a batch is grown by the host and
    the batch repeated; results identical to the roomy pool"""
    from instagraal_amd import synth
    from instagraal_amd.sampler import sampler as hip_sampler

    prob = synth.make_problem(*synth.CONFIGS["small"])
    np.random.seed(2)
    frags = np.resize(np.random.permutation(prob.n_frags), 200).astype(np.int32)
    outs = []
    for pool in (None, str(prob.n_contacts // 2), "3000"):
        if pool:
            monkeypatch.setenv("IG_POOL_ENTRIES", pool)
        s = hip_sampler(**prob.sampler_kwargs(), device_id=0)
        s.set_param_simu(prob.params)
        s.eval_likelihood_init()
        np.random.seed(3)
        cands = s.draw_candidates(frags, 5)
        res = s.ctx.step_batch(frags, cands)
        outs.append((res.tobytes(), s.gpu_vect_frags.copy_from_gpu().soa17(), s.ctx.batch_stats()["batches"]))
    for o in outs[1:]:
        assert outs[0][0] == o[0] and np.array_equal(outs[0][1], o[1])
    assert outs[1][2] > outs[0][2]  # the small pool really cut batches short


def test_slice_pool_overflow_on_the_one_move_path(monkeypatch):
    """the same for the launches of ONE move (ig_step = step_sampler, ig_score_move, ig_step_batch at width 1, ig_step_begin /
    ig_step_finish, ig_nuis_begin): a move whose lists do not fit the pool is not applied (the chooser raises a flag the apply kernels
    honour), the host grows the pool and repeats it.  Until round 4 this path scored such a move without the lists that did not fit
    (tools/fuzz_batches.py found it: nine candidates on contigs that hold a fifth of the contacts each)."""
    from instagraal_amd import hip_lib, synth
    from instagraal_amd.multi_gpu import ShardedRunner
    from instagraal_amd.sampler import sampler as hip_sampler

    prob = synth.make_problem(*synth.CONFIGS["small"])
    np.random.seed(2)
    frags = np.resize(np.random.permutation(prob.n_frags), 60).astype(np.int32)
    cols = ["o", "dist", "op_sampled", "id_f_sampled", "n_contigs"]

    class one_rank:  # (ShardedRunner's collective for a world of one)
        class ReduceOp:
            SUM = 0

        @staticmethod
        def all_reduce(t, op=None):
            return None

    outs = {}
    for pool in (None, "1024"):
        if pool:
            monkeypatch.setenv("IG_POOL_ENTRIES", pool)

        def fresh():
            s = hip_sampler(**prob.sampler_kwargs(), device_id=0)
            s.set_param_simu(prob.params)
            s.bins = np.arange(1.0, 60.0, 1.0)
            s.eval_likelihood_init()
            np.random.seed(3)
            return s

        got = {}
        s = fresh()  # step_sampler, one call per move
        got["step"] = [tuple(float(x) for x in s.step_sampler(int(f), 5)) for f in frags]
        got["step_state"] = s.gpu_vect_frags.copy_from_gpu().soa17().tobytes()
        got["retries_step"] = s.ctx.debug_pool_retries()
        s.free_gpu()
        s = fresh()  # ig_step_batch at width 1
        hip_lib.set_batch_width(1)
        try:
            cands = s.draw_candidates(frags, 5)
            got["w1"] = s.ctx.step_batch(frags, cands)[cols].tobytes()
        finally:
            hip_lib.set_batch_width(24)
        got["retries_w1"] = s.ctx.debug_pool_retries()
        s.free_gpu()
        s = fresh()  # ig_score_move (scores only), then ig_step_begin / ig_step_finish
        cands = s.draw_candidates(frags, 5)
        c0 = [int(x) for x in cands[0] if x >= 0]
        got["scores"] = s.ctx.score_move(int(frags[0]), c0).tobytes()
        got["sharded"] = ShardedRunner(s.ctx, 0, 1, dist=one_rank, tensor_factory=lambda: None)._run(frags[:20], cands[:20])[cols].tobytes()
        got["retries_sharded"] = s.ctx.debug_pool_retries()
        s.free_gpu()
        s = fresh()  # a move and the nuisance step behind it, one pair at a time (ig_nuis_begin / ig_nuis_end)
        cands = s.draw_candidates(frags, 5)
        p8 = np.array([float(s.param_simu[k][0]) for k in s.param_simu.dtype.names], np.float32)
        tup = []
        for f, cc in zip(frags[:20], cands[:20]):
            s.ctx.nuis_begin(int(f), [int(x) for x in cc if x >= 0], p8, s.mean_kb())
            r, nz, z = s.ctx.nuis_end()
            tup.append((r.o, r.dist, r.op_sampled, r.id_f_sampled, r.n_contigs, nz, z))
        got["nuis"] = repr(tup)
        got["retries_nuis"] = s.ctx.debug_pool_retries()
        s.free_gpu()
        outs[pool] = got
    a, b = outs[None], outs["1024"]
    for k in ("step", "step_state", "w1", "scores", "sharded", "nuis"):
        assert a[k] == b[k], k
    assert a["retries_step"] == a["retries_w1"] == a["retries_sharded"] == 0
    assert b["retries_step"] > 0 and b["retries_w1"] > 0 and b["retries_sharded"] > 0 and b["retries_nuis"] > 0


@pytest.mark.parametrize("way_name,window", [("plain", 48), ("plain", 0), ("nuisance", 48), ("runner", 48)])
def test_a_small_window_budget_changes_widths_not_results(way_name, window):
    """ig_debug_window_budget: the bytes the per-window arrays may take.  `small` from a bombed start -- the smallest config whose
    window strides regrow during a run (at `tiny` their 256 / 768 floors are the genome already) -- in calls of 250 moves until, under
    the default budget, the strides have regrown twice on their own (contigs of one bin merge into a few dozen; at most 8 000 moves).
    Under the default budget the buffers hold every slot they were made for; under one that holds 12 slots at the first strides (fewer
    than the default width of 24) fewer fit behind every regrowth, and still at least 2 at the end.  Every launch takes its cap from
    the slots held, so the same moves give the same records and the same genome, byte for byte, four ways (the cases): the window rule,
    plain batches (ig_set_window(0)), a run of (move, nuisance step) pairs, and multi_gpu.BatchRunner on one device sized from
    batch_max_width; the maintained sums equal a from-scratch pass."""
    from instagraal_amd import hip_lib, synth
    from instagraal_amd.multi_gpu import BatchRunner
    from instagraal_amd.sampler import sampler as hip_sampler

    prob = synth.make_problem(*synth.CONFIGS["small"])
    np.random.seed(6)
    per_call, most_calls = 250, 32
    frags = np.resize(np.random.permutation(prob.n_frags), per_call * most_calls).astype(np.int32)

    def fresh():
        s = hip_sampler(**prob.sampler_kwargs(), device_id=0)
        s.set_param_simu(prob.params)
        s.bins = np.arange(1.0, 60.0, 1.0)
        s.eval_likelihood_init()
        np.random.seed(5)
        s.bomb_the_genome()
        return s

    def plain(s, fr):
        return s.ctx.step_batch(fr, s.draw_candidates(fr, 5)).tobytes()

    def nuisance(s, fr):
        res, tuples = s.step_sampler_nuisance_batch(fr, 5, s.dt, 0, per_call * most_calls)
        return res.tobytes() + repr(tuples).encode()

    def runner(s, fr):
        return BatchRunner(s.ctx, 0, 1, width=24).run(fr, s.draw_candidates(fr, 5)).tobytes()

    s = fresh()  # the bytes of a slot at the first strides
    plain(s, frags[:2])
    held0 = s.ctx.debug_window_budget(0)
    per_slot = int(s.ctx.scratch_bytes()[0]) // held0
    s.free_gpu()
    small_budget = 12.5 * per_slot

    def run(way, window, budget, n_calls):
        """n_calls = 0: until the strides have regrown twice -> (records per call, final state, slots reported behind the first call and
        behind the last, bytes of the per-window arrays behind every call)"""
        hip_lib.set_window(window)
        s = fresh()
        s.ctx.debug_window_budget(budget)  # (no move buffers yet: the budget is set, the first call sizes them under it)
        out, window_bytes, first = [], [], 0
        while len(out) < (n_calls or most_calls):
            out.append(way(s, frags[len(out) * per_call:(len(out) + 1) * per_call]))
            if len(out) == 1:
                first = s.ctx.debug_window_budget(budget)
            window_bytes.append(int(s.ctx.scratch_bytes()[0]))  # (default budget: slots made x bytes of a slot -- it follows the strides)
            if budget:  # ig_scratch_bytes counts the slots held, not the slots asked for
                assert per_slot <= window_bytes[-1] <= budget, (window_bytes, budget)
            if not n_calls and len(set(window_bytes)) >= 3:
                break
        last = s.ctx.debug_window_budget(budget)
        sums, _ = s.ctx.debug_globals()
        _, _, limbs = s.ctx.full_likelihood(0)
        assert [int(x) for x in sums[:5]] == [int(x) for x in limbs[:5]], (way.__name__, window, budget)
        state = s.gpu_vect_frags.copy_from_gpu().soa17().tobytes()
        s.free_gpu()
        return out, state, (first, last), window_bytes

    way = {"plain": plain, "nuisance": nuisance, "runner": runner}[way_name]
    try:
        want, want_state, slots_d, bytes_d = run(way, window, 0, 0)
        got, got_state, slots_s, bytes_s = run(way, window, small_budget, len(want))
        print(way_name, window, "calls", len(want), "slots held (first, last): default budget", slots_d, "small budget", slots_s,
              "bytes of the per-window arrays: default", sorted(set(bytes_d)), "small", bytes_s)
        assert got == want and got_state == want_state
        assert len(set(bytes_d)) >= 3 and sorted(bytes_d) == bytes_d, bytes_d  # the strides regrew at least twice, on their own
        assert min(slots_d) >= 24, slots_d  # the default budget holds what the buffers were made for
        assert 2 <= slots_s[1] < slots_s[0] < 24, slots_s  # the small one fewer than the default width, fewer still at the end, never one
    finally:
        hip_lib.set_window(48)


def test_wide_slice_entries_equal_packed(monkeypatch):
    """slice entries are packed in 8 bytes when M < 2^20 and the counts are below 2^24, else kept as three ints: same results"""
    from instagraal_amd import synth
    from instagraal_amd.sampler import sampler as hip_sampler

    prob = synth.make_problem(*synth.CONFIGS["small"])
    np.random.seed(6)
    frags = np.resize(np.random.permutation(prob.n_frags), 150).astype(np.int32)
    outs = []
    for wide in ("0", "1"):
        monkeypatch.setenv("IG_WIDE_LISTS", wide)
        s = hip_sampler(**prob.sampler_kwargs(), device_id=0)
        s.set_param_simu(prob.params)
        s.eval_likelihood_init()
        np.random.seed(8)
        cands = s.draw_candidates(frags, 5)
        outs.append((s.ctx.step_batch(frags, cands).tobytes(), s.gpu_vect_frags.copy_from_gpu().soa17()))
    assert outs[0][0] == outs[1][0] and np.array_equal(outs[0][1], outs[1][1])


def test_headline_size_properties():
    """BASELINE.json's headline shape (50 k bins / 50 M contacts), where the oracle is far too slow to follow: the
    size-independent properties of the path.  (1) the incrementally maintained exact likelihood limbs equal a from-scratch
    recomputation after the run; (2) the trajectory does not depend on the batch width (24 moves per launch vs one move
    at a time): result records, final genome, stale flags; (3) the genome stays a valid set of linear contigs."""
    from instagraal_amd import hip_lib, synth
    from instagraal_amd.sampler import sampler as hip_sampler

    prob = synth.make_problem(*synth.CONFIGS["cfg3"])
    np.random.seed(0)
    frags = np.resize(np.random.permutation(prob.n_frags), 120).astype(np.int32)
    outs = []
    try:
        for W in (24, 1):
            hip_lib.set_batch_width(W)
            s = hip_sampler(**prob.sampler_kwargs(), device_id=0, coo=(prob.coo_row, prob.coo_col, prob.coo_cnt))
            s.set_param_simu(prob.params)
            s.eval_likelihood_init()
            np.random.seed(1)
            cands = s.draw_candidates(frags, 5)
            res = s.ctx.step_batch(frags, cands)
            sums, _ = s.ctx.debug_globals()
            _, _, limbs = s.ctx.full_likelihood(0)
            assert [int(x) for x in sums[:5]] == [int(x) for x in limbs[:5]], W
            st = s.gpu_vect_frags.copy_from_gpu().soa17()
            outs.append((res.tobytes(), st, [int(x) for x in s.ctx.valid_insert()]))
            s.free_gpu()
    finally:
        hip_lib.set_batch_width(24)
    assert outs[0][0] == outs[1][0]
    assert np.array_equal(outs[0][1], outs[1][1]) and outs[0][2] == outs[1][2]
    # structural validity of the final genome (names of the 17 rows: hip_lib.FRAG_FIELDS)
    f = dict(zip(hip_lib.FRAG_FIELDS, outs[0][1]))
    for cid in np.unique(f["id_c"])[:200]:
        m = np.nonzero(f["id_c"] == cid)[0]
        order = m[np.argsort(f["pos"][m])]
        assert np.array_equal(f["pos"][order], np.arange(len(m)))
        assert np.all(f["l_cont"][m] == len(m))
        assert f["prev"][order[0]] == -1 and f["next"][order[-1]] == -1
        assert np.array_equal(f["next"][order[:-1]], order[1:]) and np.array_equal(f["prev"][order[1:]], order[:-1])
        assert np.array_equal(f["start_bp"][order], np.concatenate([[0], np.cumsum(f["len_bp"][order])[:-1]]))


def test_headline_size_nuisance_run_equals_the_sequential_calls():
    """The loop with nuisance sampling at BASELINE.json's headline shape: ``step_sampler_nuisance_batch`` (moves scored ahead
    in batches across rejected steps, the pass over all 50 M contacts from tile histograms and a persistent tiled kernel,
    results through mapped host memory, the acceptance test in the library) against ``step_sampler`` +
    ``step_nuisance_parameters`` one call at a time (every column scored exactly, the plain from-scratch entry point):
    result records, nuisance tuples, parameters, generator state, genome; accepted and rejected steps, moves that conflict
    with an earlier move of their batch, winners that need the one-move tail."""
    from instagraal_amd import synth
    from instagraal_amd.sampler import sampler as hip_sampler

    prob = synth.make_problem(*synth.CONFIGS["cfg3"])
    n = 90
    outs = []
    for batch in (True, False):
        np.random.seed(21)
        s = hip_sampler(**prob.sampler_kwargs(), device_id=0, coo=(prob.coo_row, prob.coo_col, prob.coo_cnt))
        s.set_param_simu(prob.params)
        s.bins = np.arange(1.0, 60.0, 1.0)
        s.eval_likelihood_init()
        frags = np.random.permutation(prob.n_frags)[:n]
        if batch:
            b0 = s.ctx.batch_stats()
            res, tuples = s.step_sampler_nuisance_batch(frags, 5, s.dt, 0, n)
            b1 = s.ctx.batch_stats()
            assert b1["batches"] - b0["batches"] < n  # moves were scored ahead
            rows = [(float(r["o"]), float(r["dist"]), int(r["op_sampled"]), int(r["id_f_sampled"]), int(r["n_contigs"])) for r in res]
            nu = [tuple(float(np.ravel(x)[0]) for x in q[:7]) for q in tuples]
        else:
            rows, nu = [], []
            for t, f in enumerate(frags):
                r = s.step_sampler(int(f), 5, s.dt)
                rows.append((float(r[0]), float(r[1]), int(r[2]), int(r[3]), int(r[5])))
                q = s.step_nuisance_parameters(s.dt, t, n)
                nu.append(tuple(float(np.ravel(x)[0]) for x in q[:7]))
        sums, _ = s.ctx.debug_globals()
        _, _, limbs = s.ctx.full_likelihood(0)
        assert [int(x) for x in sums[:5]] == [int(x) for x in limbs[:5]]
        outs.append((rows, nu, s.gpu_vect_frags.copy_from_gpu().soa17(), np.random.get_state()[1][:6].copy(),
                     [float(s.param_simu[k][0]) for k in ("fact", "slope", "d_max", "v_inter")]))
        s.free_gpu()
        del s
    assert outs[0][0] == outs[1][0]
    assert outs[0][1] == outs[1][1]
    assert np.array_equal(outs[0][2], outs[1][2]) and np.array_equal(outs[0][3], outs[1][3]) and outs[0][4] == outs[1][4]
    assert 0 < sum(q[6] for q in outs[0][1]) < n


def test_estimate_parameters_rippe_matches_reference_golden():
    """SURVEY 8(f) f2 end to end: estimate_parameters_rippe (CL:2239-2372) on the GPU sampler against the reference's own
    method over the oracle kernels.  NOT bit for bit: the least-squares fit is ill-conditioned in the reference itself
    (three of its parameters drift with numpy's float32 code paths), so the identifiable quantities are held to tolerances
    -- slope and trans level 1e-6, the amplitude c1 * fact 1e-4, the cut-off 1e-3, the initial likelihood 1e-5."""
    from instagraal_amd import synth
    from instagraal_amd.sampler import sampler as hip_sampler

    g = np.load(os.path.join(GOLDEN, "small_estimate_mode1.npz"))
    prob = synth.make_problem(*synth.CONFIGS[str(g["config"])])
    np.random.seed(5)
    s = hip_sampler(**prob.sampler_kwargs(), device_id=0)
    s.estimate_parameters_rippe(float(g["max_dist_kb"]), float(g["size_bin_kb"]), False)
    # leastsq's (kuhn, lm, fact) are not reproducible even by the reference (ill-conditioned fit, see
    # tests/test_cpu_abi_and_host.py::test_initial_rippe_estimation_matches_reference); the identifiable quantities are:
    # slope, d, the amplitude c1 * fact * 1^slope of P(s), the cut-off, the trans level -- and through them the likelihood
    par = dict(zip(("kuhn", "lm", "c1", "slope", "d", "d_max", "fact", "v_inter"), [float(x) for x in g["params"]]))
    got = {k: float(s.param_simu[k][0]) for k in par}
    assert np.isclose(got["slope"], par["slope"], rtol=1e-6) and got["d"] == par["d"]
    assert np.isclose(got["c1"] * got["fact"], par["c1"] * par["fact"], rtol=1e-4)
    assert np.isclose(got["d_max"], par["d_max"], rtol=1e-3) and np.isclose(got["v_inter"], par["v_inter"], rtol=1e-6)
    assert np.isclose(float(s.curr_likelihood_on_nz[0]), float(g["init_nz"]), rtol=1e-5)
    # (likelihood_t is not compared: the reference's initial zero-pixel scalar is garbage, quirk Q8 / DESIGN.md section 2)


def test_batch_slots_split_over_two_ranks_equal_one_gpu():
    """multi_gpu.BatchRunner with world = 2 emulated on one GPU (two contexts, two threads, an in-process all-gather):
    each rank scores half of the slots of every batch, the records are exchanged, both commit -- results and final
    genomes identical to ig_step_batch on one context."""
    import threading

    import torch

    from instagraal_amd import synth
    from instagraal_amd.multi_gpu import BatchRunner
    from instagraal_amd.sampler import sampler as hip_sampler

    prob = synth.make_problem(*synth.CONFIGS["small"])

    def fresh():
        s = hip_sampler(**prob.sampler_kwargs(), device_id=0)
        s.set_param_simu(prob.params)
        s.eval_likelihood_init()
        return s

    np.random.seed(21)
    frags = np.resize(np.random.permutation(prob.n_frags), 300).astype(np.int32)
    ref = fresh()
    cands = ref.draw_candidates(frags, 5)
    want = ref.ctx.step_batch(frags, cands)
    want_state = ref.gpu_vect_frags.copy_from_gpu().soa17()

    world = 2
    barrier = threading.Barrier(world)
    parts = {}

    class InProcessDist:
        def __init__(self, rank):
            self.rank = rank

        def all_gather_into_tensor(self, out, mine):
            parts[(self.rank, out.numel())] = mine
            torch.cuda.synchronize()
            barrier.wait()
            chunk = mine.numel()
            for r in range(world):
                out[r * chunk:(r + 1) * chunk].copy_(parts[(r, out.numel())])
            torch.cuda.synchronize()
            barrier.wait()

    samplers = [fresh() for _ in range(world)]
    got, errs = [None] * world, []

    def work(r):
        try:
            torch.cuda.set_device(0)
            got[r] = BatchRunner(samplers[r].ctx, r, world, dist=InProcessDist(r), width=10).run(frags, cands)
        except Exception as e:  # pragma: no cover
            errs.append(e)
            barrier.abort()

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for r in range(world):
        assert got[r].tobytes() == want.tobytes(), r
        assert np.array_equal(samplers[r].gpu_vect_frags.copy_from_gpu().soa17(), want_state), r
    one = fresh()
    assert BatchRunner(one.ctx, 0, 1, width=10).run(frags, cands).tobytes() == want.tobytes()


def test_forced_apply_matches_oracle_and_keeps_sums_exact():
    """ig_apply == test_copy_struct (CL:2094-2151) for every mutation family; the maintained exact
    likelihood equals a from-scratch recomputation after each."""
    prob, s, o = make_pair("tiny")
    rng = np.random.RandomState(11)
    for op in (0, 1, 2, 5, 6, 9, 10, 12, 15, 19, 22, 23):
        a, b = rng.choice(prob.n_frags, 2, replace=False)
        max_id = o.modify_gl_cuda_buffer(int(a), o.dt)
        o.test_copy_struct(int(a), int(b), op, max_id)
        o.modify_gl_cuda_buffer(int(a), o.dt)
        s.test_copy_struct(int(a), int(b), op)
        assert np.array_equal(s.gpu_vect_frags.copy_from_gpu().soa17(), o.gpu_vect_frags.soa17()), op
        sums, _ = s.ctx.debug_globals()
        _, _, limbs = s.ctx.full_likelihood(0)
        assert [int(v) for v in sums] == [int(v) for v in limbs], op


def test_candidate_states_match_oracle():
    """All 24 candidate genomes of a move (CL:1918-1923) against the oracle's collector structs:
    every field of every fragment, contig ids up to relabelling."""
    prob, s, o = make_pair("tiny")
    rng = np.random.RandomState(2)

    def canon(ids):
        _, first = np.unique(ids, return_index=True)
        order = np.argsort(first)
        lut = {ids[first[i]]: r for r, i in enumerate(order)}
        return np.array([lut[v] for v in ids])

    for trial in range(6):
        a = int(rng.randint(prob.n_frags))
        cands = sorted(int(x) for x in rng.choice([x for x in range(prob.n_frags) if x != a], 3, replace=False))
        s.ctx.score_move(a, cands)
        o.fill_dist_single()
        max_id = o.modify_gl_cuda_buffer(a, o.dt)
        for ci, b in enumerate(cands):
            o.extract_uniq_mutations(a, b, 1 if ci == 0 else 0)
            uniq = [int(v) for v in o.gpu_list_uniq_mutations[: int(o.gpu_n_uniq[0])]]
            o.perform_mutations(a, b, max_id)
            for slot in uniq:
                got = s.ctx.debug_candidate_state(ci, slot)
                exp = o.collector_gpu_vect_frags[slot].soa17()
                for k in range(17):
                    if k == 2:
                        assert np.array_equal(canon(got[k]), canon(exp[k])), (trial, b, slot, "id_c")
                    else:
                        assert np.array_equal(got[k], exp[k]), (trial, b, slot, k)


def test_errors_are_loud():
    from instagraal_amd import hip_lib, synth
    from instagraal_amd.sampler import problem_to_context

    prob = synth.make_problem(*synth.CONFIGS["tiny"])
    ctx = problem_to_context(prob)
    with pytest.raises(hip_lib.HipError):
        ctx.step(0, [0, 5])  # candidate == focal fragment
    with pytest.raises(hip_lib.HipError):
        ctx.step(0, [prob.n_frags + 3])
    with pytest.raises(hip_lib.HipError):
        ctx.apply(1, 2, 24)
    c2 = hip_lib.Context(0)
    with pytest.raises(hip_lib.HipError):
        c2.step(0, [1])  # nothing uploaded


def test_nuisance_batch_matches_golden_and_the_sequential_calls():
    """step_sampler_nuisance_batch (the move and the nuisance step's pass over all contacts in flight together, the run's
    generator stream drawn up front in the library) against the reference-driven golden trajectory -- return tuples, nuisance
    tuples, generator state, genome -- and against the one-call-at-a-time methods on a larger problem."""
    from instagraal_amd import synth
    from instagraal_amd.sampler import sampler as hip_sampler

    g = np.load(os.path.join(GOLDEN, "tiny_nuis_mode1.npz"))
    prob = synth.make_problem(*synth.CONFIGS[str(g["config"])])
    np.random.seed(int(g["seed"]))
    s = hip_sampler(**prob.sampler_kwargs(), device_id=0)
    s.set_param_simu(prob.params)
    s.bins = np.arange(1.0, 60.0, 1.0)
    s.eval_likelihood_init()
    frags = np.arange(0, s.n_new_frags)
    np.random.shuffle(frags)
    nuis_from, n = int(g["nuis_from"]), len(g["frag"])
    assert np.array_equal(frags[:n], g["frag"])
    res0 = s.step_sampler_batch(g["frag"][:nuis_from], 5)
    res1, tuples = s.step_sampler_nuisance_batch(g["frag"][nuis_from:], 5, s.dt, nuis_from, n)
    res = np.concatenate([res0, res1])
    for t in range(n):
        r = res[t]
        got = [float(r["o"]), float(r["dist"]), float(r["op_sampled"]), float(r["id_f_sampled"]), float(np.float32(r["mean_len"])), float(r["n_contigs"])]
        assert got == list(g["ret"][t]), (t, got, list(g["ret"][t]))
    for k, q in enumerate(tuples):
        got = [float(q[0]), float(q[1]), float(q[2]), float(q[3]), float(q[4]), float(np.ravel(q[5])[0]), float(q[6])]
        assert got == list(g["nuis"][k]), (k, got, list(g["nuis"][k]))
    assert np.array_equal(np.random.get_state()[1][:8], g["rng_after"])
    assert np.array_equal(s.gpu_vect_frags.copy_from_gpu().soa17(), g["states"][-1])
    s.free_gpu()

    from instagraal_amd import hip_lib

    prob = synth.make_problem(*synth.CONFIGS["small"])
    outs = []
    # one call at a time; the run with the moves scored ahead in batches of 1 / 3 / 12 / a width that follows the run lengths
    for batch in (False, 1, 3, 12, 0):
        if batch is not False:
            hip_lib.set_nuis_width(batch)
        np.random.seed(8)
        s = hip_sampler(**prob.sampler_kwargs(), device_id=0)
        s.set_param_simu(prob.params)
        s.bins = np.arange(1.0, 60.0, 1.0)
        s.eval_likelihood_init()
        frags = np.random.permutation(prob.n_frags)[:70]
        np.random.normal()  # a cached gaussian in the generator at the start of the run
        if batch is not False:
            res, tuples = s.step_sampler_nuisance_batch(frags, 5, s.dt, 0, 70)
            rows = [(float(r["o"]), float(r["dist"]), int(r["op_sampled"]), int(r["id_f_sampled"]), int(r["n_contigs"])) for r in res]
            nu = [tuple(float(np.ravel(x)[0]) for x in q[:7]) for q in tuples]
        else:
            rows, nu = [], []
            for t, f in enumerate(frags):
                r = s.step_sampler(int(f), 5, s.dt)
                rows.append((float(r[0]), float(r[1]), int(r[2]), int(r[3]), int(r[5])))
                q = s.step_nuisance_parameters(s.dt, t, 70)
                nu.append(tuple(float(np.ravel(x)[0]) for x in q[:7]))
        sums, _ = s.ctx.debug_globals()
        _, _, limbs = s.ctx.full_likelihood(0)
        assert [int(x) for x in sums[:5]] == [int(x) for x in limbs[:5]]
        outs.append((rows, nu, s.gpu_vect_frags.copy_from_gpu().soa17(), np.random.get_state()[1][:6].copy(), np.random.get_state()[2:],
                     [float(s.param_simu[k][0]) for k in ("fact", "slope", "d_max", "v_inter")]))
        s.free_gpu()
    hip_lib.set_nuis_width(0)
    for o in outs[1:]:
        assert outs[0][0] == o[0]
        assert outs[0][1] == o[1]
        assert np.array_equal(outs[0][2], o[2]) and np.array_equal(outs[0][3], o[3]) and outs[0][4] == o[4]
        assert outs[0][5] == o[5]
    assert 0 < sum(q[6] for q in outs[0][1]) < 70  # steps were accepted and rejected: both branches are covered


def test_nuisance_run_entry_points_refuse_misuse():
    """ig_nuis_run_begin / ig_nuis_step_begin / ig_nuis_step_next: moves in order only, one step in flight, no run after
    another entry point has changed the genome."""
    from instagraal_amd import hip_lib, synth
    from instagraal_amd.sampler import PARAM_NAMES, problem_to_context

    prob = synth.make_problem(*synth.CONFIGS["tiny"])
    ctx = problem_to_context(prob)
    p8 = [np.float32(prob.params[k]) for k in PARAM_NAMES]
    frags = np.arange(6, dtype=np.int32)
    cands = np.array([[(f + 7 + 3 * q) % prob.n_frags for q in range(3)] for f in frags], np.int32)
    with pytest.raises(hip_lib.HipError, match="no run"):
        ctx.nuis_step_begin(0, p8, prob.mean_subfrag_kb)
    ctx.nuis_run_begin(frags, cands)
    with pytest.raises(hip_lib.HipError, match="expected 0"):
        ctx.nuis_step_begin(1, p8, prob.mean_subfrag_kb)
    ctx.nuis_step_begin(0, p8, prob.mean_subfrag_kb)
    with pytest.raises(hip_lib.HipError, match="not ended"):
        ctx.nuis_step_begin(1, p8, prob.mean_subfrag_kb)
    r, nz, z, acc = ctx.nuis_step_next(1e6, float("inf"), p8, None, prob.mean_subfrag_kb, True)  # no finite ratio reaches u = inf: rejected
    assert acc == 0 and r.error == 0 and np.isfinite(nz + z)
    r, nz, z, acc = ctx.nuis_step_next(1e6, 0.0, None, None, prob.mean_subfrag_kb, True)  # u = 0: accepted; no parameters for the next step
    assert acc == 1
    ctx.nuis_step_begin(2, p8, prob.mean_subfrag_kb)  # ... so the caller begins it
    ctx.nuis_end()
    ctx.step(int(frags[3]), cands[3])  # any other move ends the run
    with pytest.raises(hip_lib.HipError, match="no run"):
        ctx.nuis_step_begin(3, p8, prob.mean_subfrag_kb)
    ctx.close()


def test_initial_links_not_mutually_inverse_use_the_one_move_path():
    """The batch commit counts every genome-distance credit once by a rule on mutually inverse initial prev / next links
    (true of any genome the loader builds).  With other initial links the library applies one move at a time, refuses the
    batch entry points, and the batched methods of the sampler still return what the one-call-at-a-time methods return."""
    from instagraal_amd import hip_lib, synth
    from instagraal_amd.sampler import sampler as hip_sampler

    prob = synth.make_problem(*synth.CONFIGS["tiny"])
    outs = []
    for batch in (False, True):
        np.random.seed(11)
        s = hip_sampler(**prob.sampler_kwargs(), device_id=0)
        s.set_param_simu(prob.params)
        s.bins = np.arange(1.0, 60.0, 1.0)
        s.eval_likelihood_init()
        assert s.ctx.links_inverse()
        nxt = np.copy(s.np_init_next)
        a, b = np.nonzero(nxt >= 0)[0][:2]
        nxt[a], nxt[b] = nxt[b], nxt[a]  # next(prev(x)) != x for two fragments
        s.ctx.set_initial_genome(s.np_init_prev, nxt, s.np_init_orientable, s.id_frags_blacklisted)
        assert not s.ctx.links_inverse()
        frags = np.random.permutation(prob.n_frags)[:30]
        if batch:
            with pytest.raises(hip_lib.HipError, match="not mutually inverse"):
                s.ctx.nuis_run_begin(frags[:4].astype(np.int32), np.zeros((4, 5), np.int32))
            with pytest.raises(hip_lib.HipError, match="not mutually inverse"):
                s.ctx.batch_upload(frags[:4].astype(np.int32), np.zeros((4, 5), np.int32), 1)
            res = s.step_sampler_batch(frags[:15], 5)
            rows = [(float(r["o"]), float(r["dist"]), int(r["op_sampled"]), int(r["id_f_sampled"]), int(r["n_contigs"])) for r in res]
            res, tuples = s.step_sampler_nuisance_batch(frags[15:], 5, s.dt, 0, 15)
            rows += [(float(r["o"]), float(r["dist"]), int(r["op_sampled"]), int(r["id_f_sampled"]), int(r["n_contigs"])) for r in res]
            nu = [tuple(float(np.ravel(x)[0]) for x in q[:7]) for q in tuples]
        else:
            rows, nu = [], []
            for t, f in enumerate(frags):
                r = s.step_sampler(int(f), 5, s.dt)
                rows.append((float(r[0]), float(r[1]), int(r[2]), int(r[3]), int(r[5])))
                if t >= 15:
                    q = s.step_nuisance_parameters(s.dt, t - 15, 15)
                    nu.append(tuple(float(np.ravel(x)[0]) for x in q[:7]))
        outs.append((rows, nu, s.gpu_vect_frags.copy_from_gpu().soa17()))
        s.free_gpu()
    assert outs[0][0] == outs[1][0]
    assert outs[0][1] == outs[1][1]
    assert np.array_equal(outs[0][2], outs[1][2])
