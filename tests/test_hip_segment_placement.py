"""GPU tests of the segment placement support (ig_segment_placement, sampler.segment_placement) against the rule's host statement
(instagraal_amd.segment_placement.support_host: every site of every guest enumerated, the quadrants contact by contact) on the tables,
the state and the genome order downloaded from the same handle.  Every comparison is exact integer equality."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_hip_placement_support import _bins_by_contig, _contacts, _first_and_last_of_a_contig, _host_inputs, _sampler

pytestmark = pytest.mark.gpu

FIXTURES = ("matrix_tiny_plain", "matrix_tiny_bomb")
WINDOWS = (1, 2, 63, 64, 65, 1024)
FORMS = ("thread", "wave", "default")


def _assert_equal(got, want, what):
    from instagraal_amd import segment_placement as sp

    for k in sp.ARRAYS + ("quadrants",):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k, np.argwhere(got[k] != want[k])[:5].tolist())
    for k in sp.SCALARS:
        assert got[k] == want[k], (what, k, got[k], want[k])


def _min_hosts(w):
    """1, w and 2 w at the windows 1, 64 and 1024, the default (w) at the others"""
    return (w,) if w in (2, 63, 65) else (1, w, 2 * w) if w > 1 else (1, 2)


def _levels(s, prob, t):
    """the segment lists of the three levels and a gappy caller's list -> {name: (first, last)}, and first_bin per list"""
    from instagraal_amd import segment_placement as sp
    from instagraal_amd.junction_profile import contig_runs

    stot, contig, placed, position, parent, _ = t
    order = s.ctx.contact_map_order().astype(np.int64)
    g = s.gpu_vect_frags.copy_from_gpu()
    b = sp.bin_segments(order, parent)
    k = sp.block_segments(order, parent, g.id_c, g.ori, g.id_d, s.np_init_id_c, s.np_init_pos)
    members, start, length = contig_runs(contig, position)
    c = sp.scaffold_segments(order, np.repeat(start, length), np.repeat(start + length, length), np.asarray(stot)[members] != 0)
    return dict(bin=(b["first"], b["last"]), block=(k["first"], k["last"]), scaffold=(c["first"], c["last"]), gappy=(b["first"][1::3], b["last"][1::3])), b


def _assert_device_equals_rule(s, prob, what, windows=WINDOWS, forms=("default",), min_hosts=None, rule=None, levels=("bin", "block", "scaffold", "gappy")):
    """-> {(level, w, min_hosts): the rule's result}; every form of the scan in ``forms`` is held to it"""
    from instagraal_amd import segment_placement as sp

    t = _host_inputs(s.ctx, prob)
    lists, _ = _levels(s, prob, t)
    total = int(prob.coo_cnt.astype(np.int64).sum())
    out = {}
    for level in levels:
        first, last = lists[level]
        for w in windows:
            for mh in (_min_hosts(w) if min_hosts is None else min_hosts(w)):
                want = (rule or sp.support_host)(*t[:4], *_contacts(prob), first, last, w, mh)
                for form in forms:
                    s.ctx.debug_placement_support_form(form)
                    got = s.ctx.segment_placement(w, first, last, mh)
                    _assert_equal(got, want, (what, level, w, mh, form))
                    assert sp.observed_total(got) == total and (got["window"], got["min_hosts"], got["n_seg"]) == (w, mh, first.size)
                out[(level, w, mh)] = want
    s.ctx.debug_placement_support_form("default")
    return out


def _rows_on_both_sides(want):
    from instagraal_amd import segment_placement as sp

    n = np.diff(want["rowptr"])[want["status"] == 0]
    return bool((n <= sp.WAVE_ENTRIES).any() and (n > sp.WAVE_ENTRIES).any())


@pytest.mark.parametrize("name", FIXTURES)
def test_device_equals_the_rule_on_the_fixture_states(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    prob, s = _sampler(str(g["config"]), seed=11)
    s.ctx.upload_state(g["state"])
    s.modify_gl_cuda_buffer()
    s.eval_likelihood_init()
    res = _assert_device_equals_rule(s, prob, name, forms=FORMS)
    assert res[("bin", 64, 1)]["n_guests"] > 0 and (res[("block", 64, 1)]["best_contig"] >= 0).any() and res[("gappy", 64, 1)]["uncounted_observed"] > 0
    assert res[("block", 2, 2)]["quadrants"].any()
    if name.endswith("bomb"):  # guests that are whole contigs: no home
        assert (res[("scaffold", 64, 1)]["home_hosts"] == 0).all()
    s.free_gpu()


def test_device_equals_the_rule_on_small_fresh():
    prob, s = _sampler("small", seed=12)
    res = _assert_device_equals_rule(s, prob, "small fresh", windows=(1, 64, 1024), forms=FORMS, levels=("bin", "scaffold", "gappy"))
    assert _rows_on_both_sides(res[("bin", 64, 1)]) and res[("bin", 64, 1)]["n_guests"] == prob.n_frags
    assert (res[("scaffold", 64, 1)]["home_hosts"] == 0).all() and (res[("scaffold", 64, 1)]["best_contig"] >= 0).any()
    s.free_gpu()


def test_device_equals_the_rule_on_small_after_moves():
    prob, s = _sampler("small", seed=12)
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:300], 5)
    res = _assert_device_equals_rule(s, prob, "small after batch moves", windows=(2, 64), forms=FORMS, levels=("block", "gappy"), min_hosts=lambda w: (1, w))
    want = res[("block", 64, 1)]
    assert (want["best_contig"] >= 0).any() and (want["n_positions"] > 3).any() and want["quadrants"][:, 1].any() and 20 < want["n_seg"] < prob.n_frags
    s.free_gpu()


def test_device_equals_the_rule_on_small_after_the_bomb():
    prob, s = _sampler("small", seed=12)
    s.bomb_the_genome()
    res = _assert_device_equals_rule(s, prob, "small after the bomb", windows=(1, 64), levels=("bin", "scaffold"), min_hosts=lambda w: (1, 2))
    want = res[("scaffold", 64, 1)]
    assert want["n_contigs"] == prob.n_frags == want["n_guests"] and not want["home_hosts"].any() and (want["best_contig"] >= 0).sum() > 900
    s.free_gpu()


def test_a_state_with_a_ring():
    prob, s = _sampler("small", seed=13)
    first, last = _first_and_last_of_a_contig(prob)
    s.test_copy_struct(first, last, 10)
    s.modify_gl_cuda_buffer()
    res = _assert_device_equals_rule(s, prob, "small with a ring", windows=(64,), levels=("bin", "block"), min_hosts=lambda w: (w,))
    want = res[("bin", 64, 64)]
    assert want["ring_observed"] > 0 and (want["status"] == 2).sum() >= 3 and not want["quadrants"][want["status"] == 2].any()
    s.free_gpu()


def test_with_windows_of_1024_on_long_contigs():
    """contigs of thousands of sub-fragments: full windows of 2048 hosts.  The rule's sparse statement stands in for the dense one here
    (tests/test_segment_placement_host.py holds the two to the same bytes)"""
    from instagraal_amd import segment_placement as sp

    prob, s = _sampler("bigctg", seed=12)
    res = _assert_device_equals_rule(s, prob, "bigctg", windows=(1024,), forms=FORMS, min_hosts=lambda w: (2 * w,), rule=sp.support_sparse, levels=("gappy",))
    want = res[("gappy", 1024, 2048)]
    assert (want["best_hosts"] == 2048).any() and (want["home_hosts"] == 2048).any()
    s.free_gpu()


def test_level_bin_equals_the_placement_support_and_home_equals_the_orientation_support():
    from instagraal_amd import placement_support as ps

    prob, s = _sampler("small", seed=15)
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:200], 5)
    t = _host_inputs(s.ctx, prob)
    lists, b = _levels(s, prob, t)
    for w, mh in ((1, 1), (8, 8), (64, 1)):
        bins = s.ctx.placement_support(w, mh)
        got = s.ctx.segment_placement(w, *lists["bin"], mh)
        for k in ps.ARRAYS:
            assert got[k].dtype == bins[k].dtype and np.array_equal(got[k], bins[k][b["first_bin"]]), (w, mh, k)
        assert got["uncounted_observed"] == 0 and got["within_segment_observed"] == bins["within_bin_observed"] and got["entries"] == bins["entries"]
        assert all(got[k] == bins[k] for k in ("unplaced_observed", "ring_observed", "counted_observed", "n_contigs"))
        for level in ("bin", "block", "scaffold", "gappy"):
            got = s.ctx.segment_placement(w, *lists[level], mh)
            o = s.ctx.orientation_support(w, *lists[level], model=False)
            assert np.array_equal(got["quadrants"][:, 0, :], o["observed"]), (w, level)
    s.free_gpu()


def test_the_planted_block_on_the_device():
    """k = 4 neighbouring bins of the longest contig moved one by one behind each other to the tail of the second longest"""
    from instagraal_amd import segment_placement as sp
    from instagraal_amd.hip_lib import FRAG_FIELDS

    w, k = 8, 4
    prob, s = _sampler("small", seed=21)
    parent = prob.np_sub_frags_2_frags["x"].astype(np.int64)
    id_c = s.ctx.download_state()[FRAG_FIELDS.index("id_c")].astype(np.int64)
    seq = _bins_by_contig(s.ctx.contact_map_order().astype(np.int64), parent)
    cuts = np.concatenate([[0], np.nonzero(id_c[seq][1:] != id_c[seq][:-1])[0] + 1, [seq.size]])
    contigs = sorted((seq[a:b].tolist() for a, b in zip(cuts[:-1], cuts[1:])), key=lambda c: -len(c))
    src, dst = contigs[0], contigs[1]
    a = (len(src) - k) // 2
    block, left, right = src[a:a + k], src[a - 1], src[a + k]
    target = dst[-1]
    for b in block:
        s.apply_replay_simu(b, target, 6)
        target = b
    s.modify_gl_cuda_buffer()
    order = s.ctx.contact_map_order().astype(np.int64)
    after = _bins_by_contig(order, parent).tolist()
    i = after.index(block[0])
    assert after[i:i + k] == block and after[i - 1] == dst[-1]  # consecutive, behind the tail of the second longest
    res = s.segment_placement(level="block", window=w)
    i0 = int(np.nonzero(res["first_bin"] == block[0])[0][0])
    assert res["last_bin"][i0] == block[-1] and res["n_positions"][i0] == np.isin(parent, block).sum()  # one block of block_segments
    f0, l0 = int(res["first"][i0]), int(res["last"][i0])
    # as in the host test: the block as an explicit segment among the bins of the rest (a scaffold nobody touched is one block and a
    # whole contig: it has no home, so its ratio is inf whatever the contacts say)
    b = sp.bin_segments(order, parent)
    rest = (b["first"] < f0) | (b["first"] > l0)
    first, last = np.sort(np.concatenate([b["first"][rest], [f0]])), np.sort(np.concatenate([b["last"][rest], [l0]]))
    res = s.segment_placement(segments=(first, last), window=w)
    i0 = int(np.nonzero(res["first"] == f0)[0][0])
    assert res["level"] == "custom" and (res["first_bin"][i0], res["last_bin"][i0]) == (block[0], block[-1]) and res["n_seg"] == b["first"].size - k + 1
    t = _host_inputs(s.ctx, prob)
    _assert_equal(res, sp.support_host(*t[:4], *_contacts(prob), res["first"], res["last"], w), "planted")
    bins = s.placement_support(w)
    print("ratio", res["ratio"][i0], "second_ratio", res["second_ratio"][i0], "keep/flip", res["keep"][i0, 1], res["flip"][i0, 1], "bins", bins["ratio"][block])
    assert res["ratio"][i0] >= 10 and res["second_ratio"][i0] < 0.5
    assert res["best_contig"][i0] == bins["contig"][left] == bins["contig"][right] != res["contig"][i0]
    assert abs(int(res["best_offset"][i0]) - int(bins["offset"][right])) <= w  # the gap between its former neighbours, adjacent now
    assert res["best_scaffold"][i0] == bins["scaffold"][left] != res["scaffold"][i0] and {int(res["best_before"][i0]), int(res["best_after"][i0])} <= set(src)
    assert res["keep"][i0, 1] > res["flip"][i0, 1] and res["verdict"][i0, 1] == "as_placed"
    assert s.misplaced_segments(5, segments=(first, last), window=w)["segment"][0] == i0 == sp.misplaced_segments(res)["segment"][0]
    assert np.all(bins["ratio"][block[1:-1]] < 1)  # bin by bin the interior of the block is at home
    s.free_gpu()


def test_two_calls_agree_and_the_timed_call_reports_every_pass():
    from instagraal_amd import hip_lib, segment_placement as sp

    prob, s = _sampler("small", seed=18)
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:200], 5)
    lists, _ = _levels(s, prob, _host_inputs(s.ctx, prob))
    first, last = lists["block"]
    a, b = s.ctx.segment_placement(64, first, last), s.ctx.segment_placement(64, first, last)
    assert all(a[k].tobytes() == b[k].tobytes() for k in sp.ARRAYS + ("quadrants",)) and all(a[k] == b[k] for k in sp.SCALARS)
    sums = []
    for form in FORMS:
        s.ctx.debug_placement_support_form(form)
        ms, ck = s.ctx.debug_segment_placement_time(64, first, last, n=2)
        assert ms.shape == (2, len(hip_lib.SEGMENT_PLACEMENT_PASSES)) == (2, 11) and (ms[:, :4] > 0).all() and (ms[:, 7:] > 0).all()
        sums.append(ck)
    s.ctx.debug_placement_support_form("default")
    words = np.concatenate([a[k].astype(np.int64) for k in sp.ARRAYS] + [a["quadrants"].ravel(), np.array([a[k] for k in sp.SCALARS], np.int64)]).tolist()
    tot = sum(int(v) * (i + 1) for i, v in enumerate(words)) % (1 << 64)
    assert sums[0] == sums[1] == sums[2] == (tot - (1 << 64) if tot >= 1 << 63 else tot)
    s.free_gpu()


def test_the_calls_disturb_nothing():
    outs = []
    for with_calls in (False, True):
        prob, s = _sampler("small", seed=3)
        frags = np.random.permutation(prob.n_frags)[:200]
        res = [s.step_sampler_batch(frags[:100], 5)]
        if with_calls:
            for level in ("block", "scaffold", "bin"):
                assert s.segment_placement(level=level)["n_guests"] > 0
            r = s.segment_placement(window_kb=20.0)
            ms, _ = s.ctx.debug_segment_placement_time(1024, r["first"], r["last"], n=2)
            assert ms.shape == (2, 11) and s.misplaced_segments(5, min_ratio=0.0, level="bin").size > 0
            assert s.segment_placement(segments=(r["first"][::2], r["last"][::2]), window=8, min_hosts=1)["level"] == "custom"
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


def test_errors_are_loud_and_leave_the_context_usable():
    import ctypes as C

    from instagraal_amd import hip_lib, segment_placement as sp
    from instagraal_amd.sampler import LIST_SIZE, N_INSERT_BLOCKS, PARAM_NAMES, problem_to_context, soa17_from_dict

    prob, s = _sampler("tiny")
    lists, _ = _levels(s, prob, _host_inputs(s.ctx, prob))
    first, last = lists["block"]
    bf, bl = lists["bin"]
    T = int(bl[-1]) + 1
    ref = s.ctx.segment_placement(64, first, last)

    def ok():
        _assert_equal(s.ctx.segment_placement(64, first, last), ref, "again")

    for bad in (0, 1025, -1):
        with pytest.raises(hip_lib.HipError, match="ig_segment_placement.*window"):
            s.ctx.segment_placement(bad, first, last, 1)
        with pytest.raises(hip_lib.HipError, match="window"):
            s.ctx.debug_segment_placement_time(bad, first, last, 1)
        ok()
    for w, bad in ((64, 0), (64, 129), (1, 3), (1024, 2049), (8, -1)):
        with pytest.raises(hip_lib.HipError, match="ig_segment_placement.*min_hosts"):
            s.ctx.segment_placement(w, first, last, bad)
    ok()
    for f, l, what in ((bf[::-1], bl[::-1], "not ascending and disjoint"), (np.array([0, 3]), np.array([3, 5]), "not ascending and disjoint"),
                       (np.array([-1]), np.array([2]), "out of range"), (np.array([5]), np.array([T]), "out of range"), (np.array([5]), np.array([4]), "out of range"),
                       (np.array([0]), np.array([T - 1]), "spans two contigs"), (np.arange(T + 1), np.arange(T + 1), "out of range")):
        with pytest.raises(hip_lib.HipError, match="ig_segment_placement: segment list.*" + what):
            s.ctx.segment_placement(64, f, l)
        with pytest.raises(ValueError, match="segment placement: segment list.*" + what):  # the rule refuses in the same words
            sp.support_host(*_host_inputs(s.ctx, prob)[:4], *_contacts(prob), f, l, 64)
        ok()
    with pytest.raises(hip_lib.HipError, match="integer vectors"):
        s.ctx.segment_placement(64, np.array([0.5]), np.array([2.0]))
    n = first.size
    ints, longs, quad, sc = np.full((12, n), -7, np.int32), np.full((6, n), -7, np.int64), np.full((n, 3, 4), -7, np.int64), np.full(9, -7, np.int64)
    f32, l32 = first.astype(np.int32), last.astype(np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    fn = hip_lib.lib().ig_segment_placement
    for args, what in (((C.c_int32(n), p(f32), p(l32), C.c_void_p(0), p(longs), p(quad), p(sc)), b"NULL output"),
                       ((C.c_int32(n), p(f32), p(l32), p(ints), p(longs), C.c_void_p(0), p(sc)), b"NULL output"),
                       ((C.c_int32(n), p(f32), p(l32), p(ints), p(longs), p(quad), C.c_void_p(0)), b"NULL output"),
                       ((C.c_int32(n), C.c_void_p(0), p(l32), p(ints), p(longs), p(quad), p(sc)), b"NULL segment list"),
                       ((C.c_int32(-1), p(f32), p(l32), p(ints), p(longs), p(quad), p(sc)), b"segment list of -1 entries")):
        assert fn(s.ctx._h, C.c_int32(64), C.c_int32(64), *args) != 0 and what in hip_lib.lib().ig_last_error(), what
        assert all(np.all(a == -7) for a in (ints, longs, quad, sc))
    ok()
    # between ig_nuis_begin and ig_nuis_end the call refuses, and the step ends as if nothing had happened
    cands = s.return_neighbours(3, 5)
    p8 = np.array([float(s.param_simu[k][0]) for k in PARAM_NAMES], np.float32)
    s.ctx.nuis_begin(3, sorted(int(x) for x in cands if x != 3), p8, s.mean_kb())
    with pytest.raises(hip_lib.HipError, match="ig_segment_placement.*in flight"):
        s.ctx.segment_placement(64, first, last)
    with pytest.raises(hip_lib.HipError, match="in flight"):
        s.ctx.debug_segment_placement_time(64, first, last)
    s.ctx.nuis_end()
    ok()
    with pytest.raises(ValueError):
        s.segment_placement(window=8, window_kb=16.0)
    with pytest.raises(ValueError, match="segment placement.*min_hosts"):
        s.segment_placement(window=8, min_hosts=17)
    with pytest.raises(ValueError, match="level"):
        s.segment_placement(level="contig")
    s.free_gpu()
    # a sharded handle: the maximum needs the whole profile
    shard = problem_to_context(prob)
    shard.set_shard(0, 2)
    with pytest.raises(hip_lib.HipError, match="segment placement needs all contacts on one handle"):
        shard.segment_placement(64, first, last)
    shard.set_shard(0, 1)
    _assert_equal(shard.segment_placement(64, first, last), ref, "whole again")
    shard.close()
    # before the contacts are uploaded, before a state
    bare = hip_lib.Context(0)
    bare.upload_subfrag_table(prob.np_sub_frags_2_frags)
    with pytest.raises(hip_lib.HipError, match="contacts"):
        bare.segment_placement(64, first, last)
    bare.upload_contacts(prob.coo_row, prob.coo_col, prob.coo_cnt, prob.n_sub_frags)
    bare.set_insert_config(LIST_SIZE[:N_INSERT_BLOCKS], int(LIST_SIZE[:N_INSERT_BLOCKS].max() * np.int32(np.round(prob.S_o_A_frags["sub_len"].mean()) + 1)))
    with pytest.raises(hip_lib.HipError, match="state"):
        bare.segment_placement(64, first, last)
    bare.upload_state(soa17_from_dict(prob.S_o_A_frags, prob.n_frags))
    _assert_equal(bare.segment_placement(64, first, last), ref, "bare: no parameters needed")
    bare.close()


def test_a_chain_in_flight_refuses():
    from instagraal_amd import hip_lib
    from instagraal_amd.sampler import PARAM_NAMES

    prob, s = _sampler("tiny", seed=21)
    first, last = np.array([0, 4]), np.array([3, 5])
    p8 = np.array([float(s.param_simu[k][0]) for k in PARAM_NAMES], np.float32)
    frags = np.arange(8, dtype=np.int32)
    cands = np.array([[(x + 7 + 3 * q) % prob.n_frags for q in range(3)] for x in frags], np.int32)
    mean_kb = s.mean_kb()
    s.ctx.nuis_run_begin(frags, cands)
    s.ctx.nuis_step_begin(0, p8, mean_kb)
    s.ctx.nuis_step_next(1e6, float("inf"), None, None, mean_kb, True)  # (rejected: no finite ratio reaches u = inf)
    s.ctx.nuis_chain_begin(1, np.tile(p8, (2, 1)), np.full(2, np.inf), np.full(2, 1e6), mean_kb)
    with pytest.raises(hip_lib.HipError, match="ig_segment_placement: a chain is in flight"):
        s.ctx.segment_placement(8, first, last)
    with pytest.raises(hip_lib.HipError, match="a chain is in flight"):
        s.ctx.debug_segment_placement_time(8, first, last)
    s.ctx.nuis_chain_end()
    assert s.ctx.segment_placement(8, first, last)["n_seg"] == 2
    s.free_gpu()


def test_nothing_placed_no_contacts_and_no_segments():
    """T == 0, Z == 0 and n_seg == 0: success"""
    from instagraal_amd import hip_lib, segment_placement as sp, synth
    from instagraal_amd.sampler import LIST_SIZE, N_INSERT_BLOCKS, problem_to_context, soa17_from_dict

    prob = synth.make_problem(*synth.CONFIGS["tiny"])
    none = np.zeros(0, np.int32)
    total = int(prob.coo_cnt.astype(np.int64).sum())
    ctx = problem_to_context(prob)
    got = ctx.segment_placement(64, none, none)  # no segments: the class sums are the result
    assert got["n_seg"] == 0 == got["n_guests"] == got["entries"] and got["uncounted_observed"] == total and got["quadrants"].shape == (0, 3, 4)
    assert got["n_placed"] == prob.n_sub_frags and got["n_contigs"] > 0
    for f in range(prob.n_frags):  # nothing placed: a bin of every contig is inactive
        ctx.debug_set_bin_active(f, False)
    got = ctx.segment_placement(64, none, none)
    assert got["n_placed"] == 0 == got["n_contigs"] == got["entries"] and got["unplaced_observed"] == total
    with pytest.raises(hip_lib.HipError, match="segment list out of range"):
        ctx.segment_placement(64, np.array([0]), np.array([0]))
    ctx.close()
    bare = hip_lib.Context(0)  # no contacts at all
    bare.upload_subfrag_table(prob.np_sub_frags_2_frags)
    bare.upload_contacts(none, none, none, prob.n_sub_frags)
    bare.set_insert_config(LIST_SIZE[:N_INSERT_BLOCKS], int(LIST_SIZE[:N_INSERT_BLOCKS].max() * np.int32(np.round(prob.S_o_A_frags["sub_len"].mean()) + 1)))
    bare.upload_state(soa17_from_dict(prob.S_o_A_frags, prob.n_frags))
    t = _host_inputs(bare, prob)
    b = sp.bin_segments(bare.contact_map_order().astype(np.int64), t[4])
    first, last = b["first"][::2], b["last"][::2] + 0
    for form in FORMS:
        bare.debug_placement_support_form(form)
        got = bare.segment_placement(64, first, last)
        _assert_equal(got, sp.support_host(*t[:4], none, none, none, first, last, 64), ("no contacts", form))
        assert got["n_guests"] == first.size and not (got["best_contig"] >= 0).any() and (got["home_hosts"] > 0).all()
    bare.close()


def test_run_instagraal_save_segment_placements_writes_one_file_and_changes_nothing_else(tmp_path):
    from instagraal_amd import segment_placement as sp, synth
    from instagraal_amd.simulation import run_instagraal

    outs = []
    for k, flag in enumerate((True, False)):
        data = str(tmp_path / ("data%d" % k))  # (a folder of its own: a run leaves its pyramid in it)
        synth.write_text_dataset(data, n_contigs=10, mean_frags=110, seed=7, contacts_per_frag=40)
        np.random.seed(17)
        p2 = run_instagraal(data, os.path.join(data, "genome.fa"), output_folder=str(tmp_path / ("out%d" % k)), level=2, cycles=1, bomb=True,
                            save_segment_placements=flag)
        folder = p2.simulation.output_folder
        s = p2.simulation.sampler
        sums, ints = s.ctx.debug_globals()
        files = {name: open(os.path.join(folder, name), "rb").read() for name in sorted(os.listdir(folder))
                 if os.path.isfile(os.path.join(folder, name)) and name != "segment_placements.txt"}
        outs.append((s.gpu_vect_frags.copy_from_gpu().soa17(), sums.tolist(), ints.tolist(), np.random.get_state()[1].copy(), np.random.get_state()[2], files))
        names = [x for x in os.listdir(folder) if x.startswith("segment_placements")]
        if flag:
            assert names == ["segment_placements.txt"]
            upper = s.sparse_matrix.tocoo()
            total = int(upper.data[upper.row < upper.col].astype(np.int64).sum())
            lines = open(os.path.join(folder, "segment_placements.txt")).read().splitlines()
            titles = [ln for ln in lines if ln.startswith("# level=")]
            assert titles == ["# level=block", "# level=scaffold"] and lines[0] == titles[0] and lines[1][2:].split() == list(sp.FILE_COLUMNS)
            tails = [dict(kv.split("=") for kv in ln[2:].split()) for ln in lines if ln.startswith("# window=")]
            assert len(tails) == 2 and lines[-1].startswith("# window=64 min_hosts=64 ")
            blocks, scaffolds = (s.segment_placement(level=lv) for lv in ("block", "scaffold"))
            for tail, res in zip(tails, (blocks, scaffolds)):
                assert sum(int(tail[c]) for c in sp.OBSERVED_SCALARS) == total and int(tail["n_guests"]) == res["n_guests"] > 0
            rows = [ln.split() for ln in lines if not ln.startswith("#")]
            ranked = [s.misplaced_segments(n=r["n_seg"], result=r) for r in (blocks, scaffolds)]
            assert len(rows) == ranked[0].size + ranked[1].size and all(len(r) == len(sp.FILE_COLUMNS) for r in rows)
            assert [int(r[0]) for r in rows] == ranked[0]["segment"].tolist() + ranked[1]["segment"].tolist()
            fasta = set(ln[1:].split()[0] for ln in open(os.path.join(folder, "genome.fasta")) if ln.startswith(">"))
            assert set(r[3] for r in rows) | set(r[7] for r in rows) <= fasta and all(r[-1] in sp.VERDICTS for r in rows)
        else:
            assert names == []
        p2.simulation.release()
    a, b = outs
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2] and np.array_equal(a[3], b[3]) and a[4] == b[4]
    assert sorted(a[5]) == sorted(b[5]) and all(a[5][k] == b[5][k] for k in a[5])
