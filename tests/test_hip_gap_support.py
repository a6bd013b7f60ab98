"""GPU tests of the gap support (ig_gap_support, sampler.gap_support) against the rule's host statement
(instagraal_amd.gap_support.support_host: pair by pair, contact by contact) on the tables, the state and the genome order downloaded
from the same handle, with the two model values from the library's host-only entry (hip_lib.model_values_host).  Every comparison is
exact integer equality."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FIXTURES = ("matrix_tiny_plain", "matrix_tiny_bomb")
ALL = ("status", "geometry", "observed", "pairs", "log_q", "expected_q")
# arbitrary ascending floats, two of them beyond d_max (453.57 kb)
GAPS64 = np.concatenate([[0.0, 1.0, 1.5], 1.5 + np.cumsum(np.linspace(0.37, 14.0, 59)), [500.0, 1e6]]).astype(np.float32)
GAPS = {2: np.array([0.0, 7.25], np.float32), 5: np.array([0.0, 0.5, 3.0, 40.0, 1000.0], np.float32), 64: GAPS64}


def _sampler(cfg, seed=None):
    from instagraal_amd import synth
    from instagraal_amd.sampler import sampler as hip_sampler

    prob = synth.make_problem(*synth.CONFIGS[cfg])
    if seed is not None:
        np.random.seed(seed)
    s = hip_sampler(**prob.sampler_kwargs(), device_id=0)
    s.set_param_simu(dict(prob.params))
    s.bins = np.arange(1.0, 60.0, 1.0)
    s.eval_likelihood_init()
    return prob, s


def _host_inputs(s, prob):
    """what support_host takes, from ig_debug_tables, download_state and contact_map_order of the handle; and the state's columns"""
    from instagraal_amd.hip_lib import FRAG_FIELDS

    dist, contig, stot, rank, ln = s.ctx.debug_tables()
    state = s.ctx.download_state()
    col = {k: state[i] for i, k in enumerate(FRAG_FIELDS)}
    parent = prob.np_sub_frags_2_frags["x"].astype(np.int64)
    bad = np.unique(col["id_c"][col["activ"] != 1])
    placed = ~np.isin(col["id_c"][parent], bad)
    order = s.ctx.contact_map_order().astype(np.int64)
    position = np.full(dist.size, -1, np.int64)
    position[order] = np.arange(order.size)
    return (dist, stot, contig, placed, position), order, parent, col


def _model(s):
    """s (f32) -> (e_q, l_q) under the sampler's parameter set 0, on the CPU"""
    from instagraal_amd import hip_lib
    from instagraal_amd.sampler import PARAM_NAMES

    p8 = np.array([float(s.param_simu[k][0]) for k in PARAM_NAMES], np.float32)
    return lambda sep: hip_lib.model_values_host(p8, sep)


def _levels(s, prob):
    """the two junction lists of the state of the moment, built here from the downloaded state -> {level: table}"""
    from instagraal_amd import gap_support as gs

    _, order, parent, col = _host_inputs(s, prob)
    S0 = prob.S_o_A_frags
    return dict(bin=gs.bin_junctions(order, parent, col["id_c"]),
                block=gs.block_junctions(order, parent, col["id_c"], col["ori"], col["id_d"], S0["id_c"], S0["pos"]))


def _assert_equals_host(s, prob, what, windows, n_gaps=(5,), levels=("block", "bin"), junctions=None, lean=True):
    """the device's arrays and scalars against support_host, for every window, grid and list; -> the last result"""
    from instagraal_amd import gap_support as gs

    tables, order, parent, col = _host_inputs(s, prob)
    total = int(prob.coo_cnt.astype(np.int64).sum())
    model = _model(s)
    lists = _levels(s, prob)
    canonical = col["id_c"].astype(np.int64)[parent]
    got = None
    for level in (levels if junctions is None else ("custom",)):
        for w in windows:
            for K in n_gaps:
                gaps = GAPS[K] if K in GAPS else None
                if junctions is None:
                    got = s.gap_support(level=level, window=w, gaps_kb=gaps)
                    for k in ("junction", "left_bin", "right_bin", "scaffold"):
                        assert np.array_equal(got[k], lists[level][k]), (what, level, k)
                    if got["n_junctions"] == 0:  # (fresh: a block is its contig; behind the bomb: a bin is)
                        assert got["log_q"].shape == (0, got["gaps_kb"].size) and got["verdict"].size == 0
                        continue
                else:
                    got = s.gap_support(junctions=junctions, window=w, gaps_kb=gaps)
                want = gs.support_host(*tables, prob.coo_row, prob.coo_col, prob.coo_cnt, got["junction"], got["gaps_kb"], w, model, canonical=canonical)
                assert got["n_placed"] == want["n_placed"] == int(tables[3].sum()) and got["window"] == w and got["level"] == level
                assert got["status"].dtype == got["geometry"].dtype == np.int32 and all(got[k].dtype == np.int64 for k in ALL[2:])
                for k in ALL:
                    assert np.array_equal(got[k], want[k]), (what, level, w, K, k)
                for k in gs.SCALARS:
                    assert got[k] == want[k], (what, level, w, K, k, got[k], want[k])
                assert got["apart_q"] == want["apart_q"] and gs.observed_total(got) == total, (what, level, w)
                assert got["n_judged"] == int((got["status"] == 0).sum()) and got["contributions"] >= (got["counted"] > 0)
                idle = got["status"] != 0
                assert not any(got[k][idle].any() for k in ALL[2:]) and (got["expected_q"][~idle] > 0).all() and (got["pairs"][~idle] > 0).all()
                assert np.array_equal(got["order"], order) and set(got["verdict"].tolist()) <= {"adjacent", "gap", "apart", "none"}
                if lean:  # the model pass skipped: the rest is the same
                    raw = s.ctx.gap_support(w, got["junction"], got["gaps_kb"], model=False)
                    assert raw["expected_q"] is None and all(np.array_equal(raw[k], want[k]) for k in ALL[:5])
                    assert [raw[k] for k in gs.SCALARS] == [want[k] for k in gs.SCALARS]
    return got


@pytest.mark.parametrize("name", FIXTURES)
def test_device_equals_host_on_the_fixture_states(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    prob, s = _sampler(str(g["config"]), seed=11)
    s.ctx.upload_state(g["state"])
    s.modify_gl_cuda_buffer()
    s.eval_likelihood_init()
    got = _assert_equals_host(s, prob, name, windows=(1, 2, 8, 64), n_gaps=(2, 5, 64))
    assert got["n_junctions"] > 0 and got["counted"] > 0
    s.free_gpu()


def _spaced_junctions(start, length):
    """a custom list with junctions that are not listed in between: neighbours, steps of 3, 7 and 30 positions, in every contig"""
    out = []
    for st, n in zip(start.tolist(), length.tolist()):
        r = st + 1
        for step in (1, 1, 3, 7, 1, 30, 2):
            if r >= st + n:
                break
            out.append(r)
            r += step
    return np.array(out, np.int64)


def test_device_equals_host_on_small_fresh_after_moves_and_after_the_bomb():
    from instagraal_amd import gap_support as gs, junction_profile as jp

    prob, s = _sampler("small", seed=12)
    got = _assert_equals_host(s, prob, "small fresh", (1, 8, 64), levels=("block", "bin"))
    assert got["level"] == "bin" and got["n_judged"] == got["n_junctions"] > 800
    fresh = s.gap_support(level="bin")  # the defaults: window 64, the 32 default gaps
    assert fresh["window"] == 64 and np.array_equal(fresh["gaps_kb"], gs.default_gaps(s.mean_kb(), float(s.param_simu["d_max"][0]))) and fresh["gaps_kb"].size == 32
    assert s.gap_support()["level"] == "block"
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:300], 5)
    got = _assert_equals_host(s, prob, "small after batch moves", (1, 8, 64), n_gaps=(5, 32))
    assert _levels(s, prob)["block"]["junction"].size > 0
    tables, order, parent, col = _host_inputs(s, prob)
    _, start, length = jp.contig_runs(tables[2], tables[4])
    junc = _spaced_junctions(start, length)
    assert junc.size > 50 and {1, 3, 7, 30} <= set(np.diff(junc).tolist())
    got = _assert_equals_host(s, prob, "small, a custom list", (1, 8, 64, 256), junctions=junc)
    assert got["uncounted"] > 0 and got["counted"] > 0 and got["contributions"] > 0 and got["level"] == "custom"
    s.bomb_the_genome()  # contigs of one bin: the joins inside the bins are all there is
    got = _assert_equals_host(s, prob, "small after the bomb", (1, 8, 64))
    assert s.gap_support(level="block")["n_junctions"] == 0 and s.gap_support(level="bin")["n_junctions"] == 0
    order = s.ctx.contact_map_order().astype(np.int64)
    inside = np.nonzero(np.diff(parent[order]) == 0)[0] + 1  # (custom junctions inside the bins still work)
    _assert_equals_host(s, prob, "small after the bomb, inside the bins", (8,), junctions=inside[::5])
    s.free_gpu()


def test_full_windows_of_256_and_junctions_across_the_wave_threshold():
    from instagraal_amd import hip_lib, junction_profile as jp

    prob, s = _sampler("bigctg", seed=12)
    tables, order, parent, col = _host_inputs(s, prob)
    _, start, length = jp.contig_runs(tables[2], tables[4])
    by_len = np.argsort(-length)
    k, k2 = int(by_len[0]), int(by_len[1])
    assert length[k] >= 6600 and length[k2] >= 600
    # deep inside long contigs: both sides of the window are full at w = 256
    deep = np.sort(np.concatenate([start[k] + np.array([300, 301, 1000, 3000, 3256, 6000]), start[k2] + np.array([280, 300])]))
    K4 = np.array([0.0, 2.0, 30.0, 600.0], np.float32)
    GAPS[4] = K4
    got = _assert_equals_host(s, prob, "bigctg, full windows", (256,), n_gaps=(4,), junctions=deep, lean=False)
    assert got["geometry"][:, 1].tolist() == [256] * 8 and got["geometry"][:, 2].tolist() == [256] * 8 and (got["pairs"] == 256 * 257 // 2).all()
    # pairs * K just under, at and just over GAP_WAVE_TERMS = 8192, with K = 32: one position in front of the junction and a window
    # of 255 (255 pairs, 8160 terms) and of 256 (256 pairs, 8192 terms); two positions in front and a window of 129 (257 pairs, 8224)
    W = hip_lib.GAP_SUPPORT_WAVE_TERMS
    assert W == 8192
    for junc, w, terms in ((start[k] + 1, 255, W - 32), (start[k] + 1, 256, W), (start[k] + 2, 129, W + 32)):
        got = _assert_equals_host(s, prob, "bigctg, the threshold", (w,), n_gaps=(32,), junctions=np.array([junc, start[k] + 300]), lean=False)
        assert int(got["pairs"][0]) * 32 == terms and got["gaps_kb"].size == 32
        # every form of the model pass returns the same bytes
        cks = [s.ctx.debug_gap_support_time(w, got["junction"], got["gaps_kb"], which=form)[1] for form in ("model", "model_wave", "model_workgroup")]
        want = sum(int(v) * (i + 1) for i, v in enumerate(got["expected_q"].ravel().tolist())) % (1 << 64)
        assert cks[0] == cks[1] == cks[2] == (want - (1 << 64) if want >= 1 << 63 else want), (w, cks)
    cks = [s.ctx.debug_gap_support_time(256, deep, K4, which=form, n=2)[1] for form in ("model", "model_wave", "model_workgroup")]
    assert cks[0] == cks[1] == cks[2]
    s.free_gpu()


def test_gap_zero_is_the_junction_profile_at_the_listed_junctions():
    """an independent device path: ig_junction_profile's difference arrays and prefix sums"""
    prob, s = _sampler("small", seed=14)
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:200], 5)
    for w in (1, 8, 64, 256):
        prof = s.ctx.junction_profile(w)
        for level in ("block", "bin"):
            got = s.gap_support(level=level, window=w, gaps_kb=GAPS[5])
            j = got["junction"]
            assert (j.size > 0 or level == "block") and np.array_equal(got["observed"], prof["observed"][j]) and np.array_equal(got["pairs"], prof["pairs"][j])
            assert np.array_equal(got["expected_q"][:, 0], prof["expected_q"][j]), (w, level)
    s.free_gpu()


def _pop_a_run(prob, s, n_pop):
    """forced pop-outs (operator 0: the bin becomes a contig of its own) of n_pop consecutive bins out of the middle of the longest
    contig -> (the bin in front of the run, the bin behind it, the summed length of the popped bins in kb)"""
    S0 = prob.S_o_A_frags
    c = int(np.argmax(np.bincount(S0["id_c"])))
    fr = np.nonzero(S0["id_c"] == c)[0]
    fr = fr[np.argsort(S0["pos"][fr])]
    mid = len(fr) // 2
    popped = fr[mid:mid + n_pop]
    for a in popped.tolist():
        s.apply_replay_simu(a, int(fr[2]), 0)
        s.modify_gl_cuda_buffer()
    parent = prob.np_sub_frags_2_frags["x"]
    return int(fr[mid - 1]), int(fr[mid + n_pop]), float(prob.S_o_A_sub_frags["len_bp"][np.isin(parent, popped)].sum()) / 1000.0


def test_a_planted_gap_through_the_samplers_own_move():
    """eight consecutive bins popped out of the middle of the longest contig of ``bigctg``: the junction between the two flanks is a
    block junction whose true gap is the summed length of the popped bins (47.6 kb).  The rule's host statement on the ORACLE sampler's
    state after the same moves (window 16, the default grid) gives ll[nearest grid value, 47.9 kb] - ll[0] = 86.39 and llr_gap = 99.38
    (best 15.6 kb: the synthetic counts, 1 + Poisson(36 / s), do not follow the model's s^-1.5 law, so the size is biased low; DESIGN
    4.20)."""
    from instagraal_amd import gap_support as gs

    prob, s = _sampler("bigctg", seed=12)
    left_bin, right_bin, true_gap = _pop_a_run(prob, s, 8)
    assert 47.0 < true_gap < 48.0
    blocks = _levels(s, prob)["block"]
    hit = np.nonzero((blocks["left_bin"] == left_bin) & (blocks["right_bin"] == right_bin))[0]
    assert hit.size == 1  # it is in block_junctions
    k = int(hit[0])
    got = _assert_equals_host(s, prob, "bigctg with a planted gap", (16,), n_gaps=(32,), levels=("block",))
    nearest = int(np.argmin(np.abs(got["gaps_kb"] - true_gap)))
    print("planted gap: ll[nearest] - ll[0] = %.4f, llr_gap = %.4f, best %.4f kb, interval %.4f .. %.4f" % (
        got["ll"][k, nearest] - got["ll"][k, 0], got["llr_gap"][k], got["gap_kb"][k], got["gap_lo"][k], got["gap_hi"][k]))
    assert got["ll"][k, nearest] > got["ll"][k, 0]  # the CPU value of the difference: 86.39
    assert got["llr_gap"][k] > gs.HALF_CHI2_95 and got["verdict"][k] == "gap"  # the CPU value: 99.38
    top = s.gapped_joins(5, result=got)
    assert k in top["index"] and top["verdict"][top["index"] == k][0] == "gap"
    s.free_gpu()


def _first_and_last_of_a_contig(prob, min_frags=3):
    S = prob.S_o_A_frags
    ids, cnt = np.unique(S["id_c"], return_counts=True)
    c = ids[np.argmax(cnt >= min_frags)]
    fr = np.nonzero(S["id_c"] == c)[0]
    return int(fr[np.argmin(S["pos"][fr])]), int(fr[np.argmax(S["pos"][fr])])


def test_a_state_with_a_ring():
    """operator 10 forced on the first and the last bin of one contig closes it on itself (paste_contigs KA:3367-3693)"""
    prob, s = _sampler("small", seed=13)
    first, last = _first_and_last_of_a_contig(prob)
    s.test_copy_struct(first, last, 10)
    s.modify_gl_cuda_buffer()
    g = s.gpu_vect_frags.copy_from_gpu()
    assert (g.circ == 1).sum() >= 3 and s.ctx.debug_tables()[2].any()
    got = _assert_equals_host(s, prob, "small with a ring", (1, 8, 256), levels=("bin",))
    on_ring = g.circ[got["right_bin"]] == 1
    assert on_ring.sum() >= 2 and got["ring"] > 0
    assert set(got["status"][on_ring].tolist()) == {2} and not got["geometry"][on_ring, 1:].any() and 2 not in got["status"][~on_ring]
    assert not any(got[k][on_ring].any() for k in ALL[2:]) and set(got["verdict"][on_ring].tolist()) == {"none"}
    s.free_gpu()


def _checksum(res):
    from instagraal_amd import gap_support as gs

    words = res["observed"].tolist() + res["log_q"].ravel().tolist() + [res[k] for k in gs.SCALARS[:6]]
    tot = sum(int(v) * (j + 1) for j, v in enumerate(words)) % (1 << 64)
    return tot - (1 << 64) if tot >= 1 << 63 else tot


def test_the_time_entry_point_and_its_checksums():
    prob, s = _sampler("small", seed=15)
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:200], 5)
    lists = _levels(s, prob)
    for level in ("bin", "block"):
        j = lists[level]["junction"]
        assert j.size > 0 or level == "block"
        for w in (1, 8, 256) if j.size else ():
            ms, ck = s.ctx.debug_gap_support_time(w, j, GAPS[5], which="observed", n=2)
            res = s.ctx.gap_support(w, j, GAPS[5])
            assert ck == _checksum(res), (level, w)
            assert ms.size == 2 and (ms > 0).all()
            cks = [s.ctx.debug_gap_support_time(w, j, GAPS[5], which=form)[1] for form in ("model", "model_wave", "model_workgroup")]
            want = sum(int(v) * (i + 1) for i, v in enumerate(res["expected_q"].ravel().tolist())) % (1 << 64)
            assert cks[0] == cks[1] == cks[2] == (want - (1 << 64) if want >= 1 << 63 else want), (level, w)
    s.free_gpu()


def test_the_shards_add_up():
    from instagraal_amd import gap_support as gs, synth
    from instagraal_amd.sampler import problem_to_context

    prob = synth.make_problem(*synth.CONFIGS["small"])
    whole = problem_to_context(prob)
    parent = prob.np_sub_frags_2_frags["x"].astype(np.int64)
    junc = gs.bin_junctions(whole.contact_map_order().astype(np.int64), parent, prob.S_o_A_frags["id_c"])["junction"]
    want = whole.gap_support(8, junc, GAPS[5])
    assert want["n_judged"] == junc.size > 0 and want["counted"] > 0
    parts = []
    for rank in range(2):
        ctx = problem_to_context(prob)
        ctx.set_shard(rank, 2)
        parts.append(ctx.gap_support(8, junc, GAPS[5]))
        ctx.close()
    assert all(p["observed"].sum() > 0 for p in parts)
    for k in ("observed", "log_q"):
        assert np.array_equal(parts[0][k] + parts[1][k], want[k]), k
    for k in gs.SCALARS[:6]:
        assert parts[0][k] + parts[1][k] == want[k], k
    for p in parts:  # the model part, the pairs and the geometry whole on every rank
        assert all(np.array_equal(p[k], want[k]) for k in ("expected_q", "pairs", "geometry", "status")) and p["n_judged"] == want["n_judged"]
    whole.close()


def test_refusals_are_loud_and_leave_the_context_usable():
    from instagraal_amd import gap_support as gs, hip_lib, junction_profile as jp
    from instagraal_amd.sampler import PARAM_NAMES

    prob, s = _sampler("tiny")
    junc = _levels(s, prob)["bin"]["junction"]
    gaps = GAPS[5]
    ref = s.ctx.gap_support(8, junc, gaps)
    T, n_j = ref["n_placed"], ref["n_junctions"]

    def ok():
        again = s.ctx.gap_support(8, junc, gaps)
        assert all(np.array_equal(again[k], ref[k]) for k in ALL) and [again[k] for k in gs.SCALARS] == [ref[k] for k in gs.SCALARS]

    for bad in (0, 257, -1):
        with pytest.raises(hip_lib.HipError, match="ig_gap_support.*window"):
            s.ctx.gap_support(bad, junc, gaps)
        with pytest.raises(hip_lib.HipError, match="window"):
            s.ctx.debug_gap_support_time(bad, junc, gaps)
        with pytest.raises(ValueError, match="window"):
            s.gap_support(window=bad)
        ok()
    # the grid: too few, too many, not from 0, not ascending, not finite
    for bad in ([0.0], np.arange(65.0), [1.0, 2.0], [0.0, 2.0, 2.0], [0.0, 3.0, 1.0], [0.0, np.inf], [0.0, np.nan, 4.0]):
        with pytest.raises(hip_lib.HipError, match="ig_gap_support.*gaps"):
            s.ctx.gap_support(8, junc, np.array(bad, np.float32))
        with pytest.raises(hip_lib.HipError, match="gaps"):
            s.ctx.debug_gap_support_time(8, junc, np.array(bad, np.float32))
        with pytest.raises(ValueError, match="gaps"):
            s.gap_support(gaps_kb=bad)
        ok()
    # malformed lists: a contig boundary, descending, equal, j = 0, out of range
    tables, order, parent, col = _host_inputs(s, prob)
    _, start, length = jp.contig_runs(tables[2], tables[4])
    assert start.size >= 2 and length[0] >= 8
    edge = int(start[1])
    for bad, what in (([edge], "contig boundary"), ([2, edge, edge + 1], "contig boundary"), ([6, 3], "not strictly ascending"), ([4, 4], "not strictly ascending"),
                      ([0], "out of range"), ([0, 3], "out of range"), ([T], "out of range"), ([-1], "out of range"), ([3, T + 7], "out of range")):
        with pytest.raises(hip_lib.HipError, match="ig_gap_support: junction list.*" + what):
            s.ctx.gap_support(8, np.array(bad), gaps)
        with pytest.raises(hip_lib.HipError, match="junction list"):
            s.ctx.debug_gap_support_time(8, np.array(bad), gaps)
        ok()
    with pytest.raises(hip_lib.HipError, match="ig_gap_support: junction list"):
        s.ctx.gap_support(8, np.zeros(0, np.int64), gaps)  # n_junc < 1
    with pytest.raises(hip_lib.HipError, match="junction list"):
        s.ctx.gap_support(8, np.arange(1, T + 2), gaps)  # more junctions than positions
    ok()
    # NULL outputs: nothing is written
    lib = hip_lib.lib()
    j32 = junc.astype(np.int32)
    st, geo = np.full(n_j, -7, np.int32), np.full((n_j, 4), -7, np.int32)
    obs, prs = np.full(n_j, -7, np.int64), np.full(n_j, -7, np.int64)
    lgq, exq, sc = np.full((n_j, 5), -7, np.int64), np.full((n_j, 5), -7, np.int64), np.full(8, -7, np.int64)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    null = C.c_void_p(0)
    head = (s.ctx._h, C.c_int32(8), C.c_int32(1), C.c_int32(n_j))
    outs = [p(st), p(geo), p(obs), p(prs), p(lgq), p(exq), p(sc)]
    for k in range(7):
        args = list(outs)
        args[k] = null
        assert lib.ig_gap_support(*head, p(j32), C.c_int32(5), p(gaps), *args) != 0 and b"NULL" in lib.ig_last_error()
        assert all(np.all(x == -7) for x in (st, geo, obs, prs, lgq, exq, sc))
    assert lib.ig_gap_support(*head, null, C.c_int32(5), p(gaps), *outs) != 0 and b"NULL" in lib.ig_last_error()
    assert lib.ig_gap_support(*head, p(j32), C.c_int32(5), null, *outs) != 0 and b"NULL" in lib.ig_last_error()
    assert all(np.all(x == -7) for x in (st, geo, obs, prs, lgq, exq, sc))
    # model == 0: expected_q may be NULL
    args = list(outs)
    args[5] = null
    assert lib.ig_gap_support(s.ctx._h, C.c_int32(8), C.c_int32(0), C.c_int32(n_j), p(j32), C.c_int32(5), p(gaps), *args) == 0
    assert all(np.array_equal(x, ref[k]) for x, k in ((st, "status"), (geo, "geometry"), (obs, "observed"), (prs, "pairs"), (lgq, "log_q"))) and np.all(exq == -7)
    # a parameter set whose values times the pairs of a window could overflow the 64-bit sum: refused, not wrapped
    vals = [np.float32(s.param_simu[k][0]) for k in PARAM_NAMES]
    huge = list(vals)
    huge[PARAM_NAMES.index("fact")] = np.float32(vals[PARAM_NAMES.index("fact")] * 1e12)
    s.ctx.set_params(huge, s.mean_kb(), 0)
    with pytest.raises(hip_lib.HipError, match="model value too large for this window"):
        s.ctx.gap_support(256, junc, gaps)
    with pytest.raises(hip_lib.HipError, match="model value too large for this window"):
        s.ctx.debug_gap_support_time(256, junc, gaps, which="model")
    s.ctx.set_params(vals, s.mean_kb(), 0)
    ok()
    # no contacts uploaded
    bare = hip_lib.Context(0)
    bare.upload_subfrag_table(prob.np_sub_frags_2_frags)
    with pytest.raises(hip_lib.HipError, match="ig_gap_support.*contacts"):
        bare.gap_support(8, junc, gaps)
    bare.close()
    # between ig_nuis_begin and ig_nuis_end the call refuses, and the step ends as if nothing had happened
    cands = s.return_neighbours(3, 5)
    p8 = np.array([float(s.param_simu[k][0]) for k in PARAM_NAMES], np.float32)
    s.ctx.nuis_begin(3, sorted(int(x) for x in cands if x != 3), p8, s.mean_kb())
    with pytest.raises(hip_lib.HipError, match="ig_gap_support.*in flight"):
        s.ctx.gap_support(8, junc, gaps)
    with pytest.raises(hip_lib.HipError, match="in flight"):
        s.ctx.debug_gap_support_time(8, junc, gaps)
    s.ctx.nuis_end()
    assert s.ctx.gap_support(8, _levels(s, prob)["bin"]["junction"], gaps)["n_placed"] == T
    s.free_gpu()


def test_a_chain_in_flight_refuses():
    from instagraal_amd import hip_lib
    from instagraal_amd.sampler import PARAM_NAMES

    prob, s = _sampler("tiny", seed=21)
    junc = _levels(s, prob)["bin"]["junction"]
    p8 = np.array([float(s.param_simu[k][0]) for k in PARAM_NAMES], np.float32)
    frags = np.arange(8, dtype=np.int32)
    cands = np.array([[(x + 7 + 3 * q) % prob.n_frags for q in range(3)] for x in frags], np.int32)
    mean_kb = s.mean_kb()
    s.ctx.nuis_run_begin(frags, cands)
    s.ctx.nuis_step_begin(0, p8, mean_kb)
    s.ctx.nuis_step_next(1e6, float("inf"), None, None, mean_kb, True)  # (rejected: no finite ratio reaches u = inf)
    s.ctx.nuis_chain_begin(1, np.tile(p8, (2, 1)), np.full(2, np.inf), np.full(2, 1e6), mean_kb)
    with pytest.raises(hip_lib.HipError, match="ig_gap_support: a chain is in flight"):
        s.ctx.gap_support(8, junc, GAPS[5])
    with pytest.raises(hip_lib.HipError, match="a chain is in flight"):
        s.ctx.debug_gap_support_time(8, junc, GAPS[5])
    s.ctx.nuis_chain_end()
    junc = _levels(s, prob)["bin"]["junction"]
    assert s.ctx.gap_support(8, junc, GAPS[5])["n_junctions"] == junc.size
    s.free_gpu()


def test_the_report_disturbs_nothing():
    outs = []
    for with_report in (False, True):
        prob, s = _sampler("small", seed=3)
        frags = np.random.permutation(prob.n_frags)[:200]
        res = [s.step_sampler_batch(frags[:100], 5)]
        if with_report:
            bins = s.gap_support(level="bin", window=8)
            blocks = s.gap_support()
            assert blocks["window"] == 64 and blocks["level"] == "block" and blocks["n_junctions"] < bins["n_junctions"] and bins["observed"].sum() > 0
            s.gap_support(level="bin", window_kb=20.0, model=False)
            s.gapped_joins(5)
            for which in ("observed", "model", "model_wave", "model_workgroup"):
                s.ctx.debug_gap_support_time(64, bins["junction"], blocks["gaps_kb"], which=which, n=2)
        res.append(s.step_sampler_batch(frags[100:], 5))
        sums, ints = s.ctx.debug_globals()
        _, _, limbs = s.ctx.full_likelihood(0)
        assert [int(x) for x in sums[:5]] == [int(x) for x in limbs[:5]]
        outs.append((np.concatenate(res).tobytes(), s.gpu_vect_frags.copy_from_gpu().soa17(), sums.tolist(), ints.tolist(),
                     np.random.get_state()[1].copy(), np.random.get_state()[2], [int(x) for x in s.ctx.valid_insert()]))
        s.free_gpu()
    a, b = outs
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3]
    assert np.array_equal(a[4], b[4]) and a[5] == b[5] and a[6] == b[6]


def test_run_instagraal_save_gaps_writes_one_file_and_changes_nothing_else(tmp_path):
    from instagraal_amd import gap_support as gs, synth
    from instagraal_amd.simulation import run_instagraal

    outs = []
    for k, flag in enumerate((True, False)):
        data = str(tmp_path / ("data%d" % k))  # (a folder of its own: a run leaves its pyramid in it)
        synth.write_text_dataset(data, n_contigs=10, mean_frags=110, seed=7, contacts_per_frag=40)
        np.random.seed(17)
        p2 = run_instagraal(data, os.path.join(data, "genome.fa"), output_folder=str(tmp_path / ("out%d" % k)), level=2, cycles=1, bomb=True, save_gaps=flag)
        folder = p2.simulation.output_folder
        s = p2.simulation.sampler
        sums, ints = s.ctx.debug_globals()
        files = {}
        for name in sorted(os.listdir(folder)):
            path = os.path.join(folder, name)
            if os.path.isfile(path) and name != "gaps.txt":
                files[name] = open(path, "rb").read()
        outs.append((s.gpu_vect_frags.copy_from_gpu().soa17(), sums.tolist(), ints.tolist(), np.random.get_state()[1].copy(), np.random.get_state()[2],
                     [int(x) for x in s.ctx.valid_insert()], files))
        names = [x for x in os.listdir(folder) if x.startswith("gaps")]
        if flag:
            assert names == ["gaps.txt"]
            upper = s.sparse_matrix.tocoo()
            total = int(upper.data[upper.row < upper.col].astype(np.int64).sum())  # what the device holds: the strict upper triangle
            lines = open(os.path.join(folder, "gaps.txt")).read().splitlines()
            titles = [ln for ln in lines if ln.startswith("# level=")]
            assert titles == ["# level=block", "# level=bin"] and lines[0] == titles[0] and lines[1][2:].split() == list(gs.COLUMNS)
            tails = [dict(kv.split("=") for kv in ln[2:].split()) for ln in lines if ln.startswith("# window=")]
            assert len(tails) == 2 and lines[-1].startswith("# window=64 ")
            blocks, bins = (s.gap_support(level=lv) for lv in ("block", "bin"))
            for tail, res in zip(tails, (blocks, bins)):
                assert int(tail["n_junctions"]) == res["n_junctions"] and int(tail["n_judged"]) == res["n_judged"] and int(tail["n_gaps"]) == 32
                assert res["n_junctions"] == 0 or sum(int(tail[c]) for c in gs.CLASS_SCALARS) == total
            rows = [ln.split() for ln in lines if not ln.startswith("#")]
            assert len(rows) == blocks["n_junctions"] + bins["n_junctions"] > 0 and all(len(r) == len(gs.COLUMNS) for r in rows)
            for r, i in zip(rows[:blocks["n_junctions"]], range(blocks["n_junctions"])):
                assert [int(x) for x in r[:5]] == [blocks[c][i] for c in ("scaffold", "left_bin", "right_bin", "observed", "pairs")] and r[10] == blocks["verdict"][i]
        else:
            assert names == []
        p2.simulation.release()
    a, b = outs
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2] and np.array_equal(a[3], b[3]) and a[4] == b[4] and a[5] == b[5]
    assert sorted(a[6]) == sorted(b[6]) and all(a[6][n] == b[6][n] for n in a[6]), [n for n in a[6] if a[6][n] != b[6].get(n)]
