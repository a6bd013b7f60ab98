"""GPU tests of the placement support (ig_placement_support, sampler.placement_support) against the rule's host statement
(instagraal_amd.placement_support.support_host: every site of every guest enumerated) on the tables, the state and the genome order
downloaded from the same handle.  Every comparison is exact integer equality."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FIXTURES = ("matrix_tiny_plain", "matrix_tiny_bomb")
WINDOWS = (1, 2, 63, 64, 65, 1024)
FORMS = ("thread", "wave", "default")


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


def _host_inputs(ctx, prob):
    """what support_host takes in front of the contacts, from ig_debug_tables, download_state and contact_map_order of the handle"""
    from instagraal_amd.hip_lib import FRAG_FIELDS

    dist, contig, stot, rank, ln = ctx.debug_tables()
    state = ctx.download_state()
    col = {k: state[i] for i, k in enumerate(FRAG_FIELDS)}
    parent = prob.np_sub_frags_2_frags["x"].astype(np.int64)
    bad = np.unique(col["id_c"][col["activ"] != 1])
    placed = ~np.isin(col["id_c"][parent], bad)
    order = ctx.contact_map_order().astype(np.int64)
    position = np.full(dist.size, -1, np.int64)
    position[order] = np.arange(order.size)
    return stot, contig, placed, position, parent, prob.n_frags


def _contacts(prob):
    return prob.coo_row, prob.coo_col, prob.coo_cnt


def _assert_equal(got, want, what):
    from instagraal_amd import placement_support as ps

    for k in ps.ARRAYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k, np.nonzero(got[k] != want[k])[0][:5])
    for k in ps.SCALARS:
        assert got[k] == want[k], (what, k, got[k], want[k])


def _min_hosts(w):
    """1, w and 2 w at the windows 1, 64 and 1024, the default (w) at the others"""
    return (w,) if w in (2, 63, 65) else (1, w, 2 * w) if w > 1 else (1, 2)


def _assert_device_equals_rule(s, prob, what, windows=WINDOWS, forms=("default",), min_hosts=None, rule=None):
    """-> {(w, min_hosts): the rule's result}; every form of the scan in ``forms`` is held to it"""
    from instagraal_amd import placement_support as ps

    t = _host_inputs(s.ctx, prob)
    total = int(prob.coo_cnt.astype(np.int64).sum())
    out = {}
    for w in windows:
        for mh in (_min_hosts(w) if min_hosts is None else min_hosts(w)):
            want = (rule or ps.support_host)(*t, *_contacts(prob), w, mh)
            for form in forms:
                s.ctx.debug_placement_support_form(form)
                got = s.ctx.placement_support(w, mh)
                _assert_equal(got, want, (what, w, mh, form))
                assert ps.observed_total(got) == total and got["entries"] % 2 == 0 and (got["window"], got["min_hosts"]) == (w, mh)
            out[(w, mh)] = want
    s.ctx.debug_placement_support_form("default")
    return out


def _rows_on_both_sides(want):
    from instagraal_amd import placement_support as ps

    n = np.diff(want["rowptr"])[want["status"] == 0]
    return bool((n <= ps.WAVE_ENTRIES).any() and (n > ps.WAVE_ENTRIES).any())


@pytest.mark.parametrize("name", FIXTURES)
def test_device_equals_the_rule_on_the_fixture_states(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    prob, s = _sampler(str(g["config"]), seed=11)
    s.ctx.upload_state(g["state"])
    s.modify_gl_cuda_buffer()
    s.eval_likelihood_init()
    res = _assert_device_equals_rule(s, prob, name, forms=FORMS)
    assert res[(64, 1)]["n_guests"] > 0 and (res[(64, 1)]["best_contig"] >= 0).any()
    if name.endswith("bomb"):  # guests that are whole contigs: no home
        assert (res[(64, 1)]["home_hosts"][res[(64, 1)]["status"] == 0] == 0).any()
    s.free_gpu()


def test_device_equals_the_rule_on_small_fresh():
    prob, s = _sampler("small", seed=12)
    res = _assert_device_equals_rule(s, prob, "small fresh", forms=FORMS)
    want = res[(64, 1)]
    assert _rows_on_both_sides(want) and want["n_guests"] == prob.n_frags
    has = want["best_contig"] >= 0
    n_red = want["contig_positions"][np.maximum(want["best_contig"], 0)] - np.where(want["best_contig"] == want["contig"], want["n_positions"], 0)
    assert np.any(has & (want["best_offset"] < 64) & (want["best_hosts"] < 128)) and np.any(has & (want["best_offset"] > n_red - 64) & (want["best_hosts"] < 128))
    assert not (res[(1024, 2048)]["best_contig"] >= 0).any() and (want["second_contig"] >= 0).any()  # rows with no eligible site; runner-ups
    s.free_gpu()


def test_device_equals_the_rule_on_small_after_moves():
    prob, s = _sampler("small", seed=12)
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:300], 5)
    res = _assert_device_equals_rule(s, prob, "small after batch moves", windows=(1, 64, 1024), forms=FORMS)
    assert _rows_on_both_sides(res[(64, 1)]) and (res[(64, 64)]["best_contig"] >= 0).any()
    s.free_gpu()


def test_device_equals_the_rule_on_small_after_the_bomb():
    """contigs of one bin: no guest has a home, every window is clipped on both sides"""
    prob, s = _sampler("small", seed=12)
    s.bomb_the_genome()
    res = _assert_device_equals_rule(s, prob, "small after the bomb", windows=(1, 2, 64), forms=FORMS, min_hosts=lambda w: tuple(m for m in (1, 2, 3) if m <= 2 * w))
    want = res[(64, 1)]
    assert want["n_contigs"] == prob.n_frags == want["n_guests"] and not want["home_hosts"].any() and (want["best_contig"] >= 0).sum() > 900
    assert not (res[(64, 3)]["best_contig"] >= 0).any() or int(want["n_positions"].max()) >= 3  # (a bin of three sub-fragments hosts three)
    s.free_gpu()


def _first_and_last_of_a_contig(prob, min_frags=3):
    S = prob.S_o_A_frags
    ids, cnt = np.unique(S["id_c"], return_counts=True)
    c = ids[np.argmax(cnt >= min_frags)]
    fr = np.nonzero(S["id_c"] == c)[0]
    return int(fr[np.argmin(S["pos"][fr])]), int(fr[np.argmax(S["pos"][fr])])


def test_a_state_with_a_ring():
    """operator 10 forced on the first and the last bin of one contig closes it on itself: its bins are no guests, its contacts ``ring``"""
    prob, s = _sampler("small", seed=13)
    fresh = s.ctx.placement_support(64)
    first, last = _first_and_last_of_a_contig(prob)
    s.test_copy_struct(first, last, 10)
    s.modify_gl_cuda_buffer()
    assert (s.gpu_vect_frags.copy_from_gpu().circ == 1).sum() >= 3
    res = _assert_device_equals_rule(s, prob, "small with a ring", windows=(1, 64, 1024), min_hosts=lambda w: (w,))
    want = res[(64, 64)]
    assert want["ring_observed"] > 0 and (want["status"] == 2).sum() >= 3 and want["n_contigs"] == fresh["n_contigs"] - 1
    s.free_gpu()


def test_a_state_with_an_unplaced_contig():
    from instagraal_amd.hip_lib import FRAG_FIELDS

    prob, s = _sampler("small", seed=14)
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:100], 5)
    before = s.ctx.placement_support(64)
    id_c = s.ctx.download_state()[FRAG_FIELDS.index("id_c")]
    ids, n = np.unique(id_c, return_counts=True)
    members = np.nonzero(id_c == ids[np.argmax(n >= 3)])[0]
    s.ctx.debug_set_bin_active(members[1], False)
    res = _assert_device_equals_rule(s, prob, "small with an unplaced contig", windows=(1, 64, 1024), min_hosts=lambda w: (w,))
    want = res[(64, 64)]
    assert want["unplaced_observed"] > 0 and (want["status"] == 1).sum() == members.size and want["n_contigs"] == before["n_contigs"] - 1
    s.ctx.debug_set_bin_active(members[1], True)
    _assert_equal(s.ctx.placement_support(64), before, "the contig placed again")
    s.free_gpu()


def test_with_windows_of_1024_on_long_contigs():
    """contigs of thousands of sub-fragments: full windows of 2048 hosts, rows on both sides of the threshold of the scan's forms.  The
    rule's sparse statement stands in for the dense one here (tests/test_placement_support_host.py holds the two to the same bytes)"""
    from instagraal_amd import placement_support as ps

    prob, s = _sampler("bigctg", seed=12)
    res = _assert_device_equals_rule(s, prob, "bigctg", windows=(1024,), forms=FORMS, min_hosts=lambda w: (2 * w,), rule=ps.support_sparse)
    want = res[(1024, 2048)]
    assert _rows_on_both_sides(want) and (want["best_hosts"] == 2048).any() and (want["home_hosts"] == 2048).any()
    s.free_gpu()


def test_every_sort_form_is_reached_under_the_limits():
    """the limits of ig_debug_assembly_contacts_limits reach this feature's sorts: every form under the limits, the rows each form took
    are the ones the rule's entries per row say, and the arrays do not change"""
    from instagraal_amd import placement_support as ps

    prob, s = _sampler("tiny", seed=16)
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:100], 5)
    want = ps.support_host(*_host_inputs(s.ctx, prob), *_contacts(prob), 64, 1)
    n = want["row_entries"]
    assert int(n.sum()) == want["entries"] > int(want["rowptr"][-1])  # the reduction has equal columns to sum
    used = {k: 0 for k in ("short", "lds", "long")}
    for limits in ((0, 0), (2, 4), (1, 1), (2, 64)):
        short_max, lds_max = limits if limits != (0, 0) else (64, 1024)
        s.ctx.debug_assembly_contacts_limits(*limits)
        for form in FORMS:
            s.ctx.debug_placement_support_form(form)
            _assert_equal(s.ctx.placement_support(64, 1), want, (limits, form))
        forms = s.ctx.debug_placement_support_forms()
        rows = dict(short=(n >= 2) & (n <= short_max), lds=(n >= 2) & (n > short_max) & (n <= lds_max), long=(n >= 2) & (n > short_max) & (n > lds_max))
        for k in used:
            assert forms[k] == (int(rows[k].sum()), int(n[rows[k]].sum())), (limits, k, forms)
            used[k] += forms[k][0]
    assert all(v > 0 for v in used.values()), used
    s.ctx.debug_assembly_contacts_limits(0, 0)
    s.ctx.debug_placement_support_form("default")
    s.free_gpu()


def _bins_by_contig(order, parent):
    """the genome as lists of bins in order, one per run of the contig labels given by position"""
    bins = parent[order]
    keep = np.concatenate([[True], bins[1:] != bins[:-1]])
    return bins[keep]


def _planted(s, prob):
    """forces the (lower) middle bin of the longest contig behind the last bin of the second longest (operator 6: pop out, insert at
    the right of) -> (the moved bin as identified from the states, the bins that were its neighbours)"""
    from instagraal_amd.hip_lib import FRAG_FIELDS

    parent = prob.np_sub_frags_2_frags["x"].astype(np.int64)

    def genome():
        id_c = s.ctx.download_state()[FRAG_FIELDS.index("id_c")].astype(np.int64)
        seq = _bins_by_contig(s.ctx.contact_map_order().astype(np.int64), parent)
        cuts = np.concatenate([[0], np.nonzero(id_c[seq][1:] != id_c[seq][:-1])[0] + 1, [seq.size]])
        return [seq[a:b].tolist() for a, b in zip(cuts[:-1], cuts[1:])]

    before = genome()
    by_len = sorted(range(len(before)), key=lambda k: -len(before[k]))
    src, dst = before[by_len[0]], before[by_len[1]]
    mid = (len(src) - 1) // 2
    s.apply_replay_simu(src[mid], dst[-1], 6)
    s.modify_gl_cuda_buffer()
    after = genome()
    mates_before = {b: set(c) for c in before for b in c}
    mates_after = {b: set(c) for c in after for b in c}
    moved = [b for b in mates_before if len(mates_before[b]) > 1 and not (mates_before[b] & mates_after[b]) - {b}]
    assert moved == [src[mid]], (moved, src[mid])
    assert dst[-1] in mates_after[moved[0]] and mates_after[src[mid - 1]] == set(src) - {src[mid]}
    return moved[0], src[mid - 1], src[mid + 1]


@pytest.mark.parametrize("cfg,windows", [("tiny", (4,)), ("small", (8, 32))])
def test_the_planted_misplacement_on_the_device(cfg, windows):
    from instagraal_amd import placement_support as ps

    prob, s = _sampler(cfg, seed=21)
    for w in windows:
        assert not np.any(s.placement_support(w)["ratio"] > 1)  # fresh: nowhere denser than at home
    moved, left, right = _planted(s, prob)
    res = _assert_device_equals_rule(s, prob, "planted", windows=windows, forms=FORMS, min_hosts=lambda w: (w,))
    for w in windows:
        got = s.placement_support(w)
        _assert_equal(got, res[(w, w)], ("sampler", w))
        assert np.nonzero(got["ratio"] > 1)[0].tolist() == [moved]
        assert got["best_contig"][moved] == got["contig"][left] == got["contig"][right] != got["contig"][moved]
        former = max(int(got["offset"][left]), int(got["offset"][right]))  # the gap between its former neighbours, adjacent now
        assert abs(int(got["best_offset"][moved]) - former) <= w
        assert {int(got["best_before"][moved]), int(got["best_after"][moved])} <= set(np.nonzero(got["contig"] == got["contig"][left])[0].tolist())
        assert got["best_scaffold"][moved] == got["scaffold"][left] != got["scaffold"][moved]
        assert s.misplaced_bins(5, window=w)["bin"].tolist() == [moved] and ps.misplaced_bins(got)["best_scaffold"].tolist() == [got["scaffold"][left]]
    s.free_gpu()


def test_window_sums_against_the_lift_as_an_independent_device_path():
    """the left and right sums of home, best and runner-up recomputed on the host from the contacts in genome coordinates
    (ig_assembly_contacts_build, level "sub") of the same handle: nothing shared with the emit pass but the contacts"""
    from instagraal_amd import assembly_contacts as ac, placement_support as ps

    prob, s = _sampler("small", seed=17)
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:300], 5)
    lift = s.ctx.assembly_contacts("sub")
    pb, cnt = s.ctx.assembly_contacts_fetch(0, lift["n_entries"])
    s.ctx.assembly_contacts_release()
    pa, pb = ac.rows_of(lift["rowptr"]), pb.astype(np.int64)
    order = s.ctx.contact_map_order().astype(np.int64)
    T = order.size
    D0 = np.zeros((T, T), np.int64)
    np.add.at(D0, (pa, pb), cnt)
    D0 = D0 + D0.T
    bin_at = prob.np_sub_frags_2_frags["x"].astype(np.int64)[order]
    for w, mh in ((1, 1), (64, 64), (1024, 1)):
        got = s.ctx.placement_support(w, mh)
        start, n = ps.contig_table(got, order, prob.np_sub_frags_2_frags["x"].astype(np.int64))
        on_ring = np.isin(bin_at, np.nonzero(got["status"] != 0)[0])  # (everything is placed: a bin that is no guest is on a ring)
        assert got["n_guests"] + int((got["status"] == 2).sum()) == prob.n_frags and got["n_guests"] > prob.n_frags // 2
        D = D0.copy()
        D[on_ring, :] = 0
        D[:, on_ring] = 0
        checked = 0
        for g in np.nonzero(got["status"] == 0)[0].tolist():
            mine = np.nonzero(bin_at == g)[0]
            row = D[mine].sum(axis=0)
            row[mine] = 0
            assert (got["n_positions"][g], got["offset"][g]) == (mine.size, mine[0] - start[got["contig"][g]])
            for which in ("home", "best", "second"):
                k = got["contig"][g] if which == "home" else got[which + "_contig"][g]
                if k < 0:
                    continue
                u = int(got["offset"][g] if which == "home" else got[which + "_offset"][g])
                reduced = np.delete(row, mine)
                s0 = start[k] - (mine.size if start[k] > mine[0] else 0)
                n_red = n[k] - (mine.size if k == got["contig"][g] else 0)
                lo, hi = max(0, u - w), min(n_red, u + w)
                assert (got[which + "_left"][g], got[which + "_right"][g], got[which + "_hosts"][g]) == \
                    (reduced[s0 + lo:s0 + u].sum(), reduced[s0 + u:s0 + hi].sum(), hi - lo), (w, g, which)
                checked += 1
        assert checked > got["n_guests"]  # (home for every guest, and best sites)
        assert 2 * got["counted_observed"] == int(D.sum()) - sum(int(D[np.ix_(bin_at == g, bin_at == g)].sum()) for g in range(prob.n_frags))
    s.free_gpu()


def test_two_calls_agree_and_the_timed_call_reports_every_pass():
    from instagraal_amd import hip_lib, placement_support as ps

    prob, s = _sampler("small", seed=18)
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:200], 5)
    a, b = s.ctx.placement_support(64), s.ctx.placement_support(64)
    assert all(a[k].tobytes() == b[k].tobytes() for k in ps.ARRAYS) and all(a[k] == b[k] for k in ps.SCALARS)
    sums = []
    for form in FORMS:
        s.ctx.debug_placement_support_form(form)
        ms, ck = s.ctx.debug_placement_support_time(64, n=2)
        assert ms.shape == (2, len(hip_lib.PLACEMENT_SUPPORT_PASSES)) and (ms[:, :4] > 0).all() and (ms[:, 7:] > 0).all()
        sums.append(ck)
    s.ctx.debug_placement_support_form("default")
    words = np.concatenate([a[k].astype(np.int64) for k in ps.ARRAYS]).tolist()
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
            assert s.ctx.placement_support(64)["n_guests"] > 0
            ms, _ = s.ctx.debug_placement_support_time(1024, n=2)
            assert ms.shape == (2, 10)
            assert s.placement_support(window_kb=20.0)["n_guests"] > 0 and s.misplaced_bins(5, min_ratio=0.0).size > 0
            s.ctx.placement_support(8, 1)
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

    from instagraal_amd import hip_lib, placement_support as ps, synth
    from instagraal_amd.sampler import LIST_SIZE, N_INSERT_BLOCKS, PARAM_NAMES, problem_to_context, soa17_from_dict

    prob, s = _sampler("tiny")
    ref = s.ctx.placement_support(64)

    def ok():
        _assert_equal(s.ctx.placement_support(64), ref, "again")

    for bad in (0, 1025, -1):
        with pytest.raises(hip_lib.HipError, match="ig_placement_support.*window"):
            s.ctx.placement_support(bad, 1)
        with pytest.raises(hip_lib.HipError, match="window"):
            s.ctx.debug_placement_support_time(bad, 1)
        ok()
    for w, bad in ((64, 0), (64, 129), (1, 3), (1024, 2049), (8, -1)):
        with pytest.raises(hip_lib.HipError, match="ig_placement_support.*min_hosts"):
            s.ctx.placement_support(w, bad)
    ok()
    with pytest.raises(hip_lib.HipError, match="form"):
        hip_lib._ck(hip_lib.lib().ig_debug_placement_support_form(s.ctx._h, C.c_int32(3)))
    arrays = [np.zeros(prob.n_frags, np.int32 if k in ps.INT_ARRAYS else np.int64) for k in ps.ARRAYS]
    sc = np.full(7, -7, np.int64)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    args = [p(a) for a in arrays]
    args[5] = C.c_void_p(0)
    assert hip_lib.lib().ig_placement_support(s.ctx._h, C.c_int32(64), C.c_int32(64), *args, p(sc)) != 0 and b"NULL" in hip_lib.lib().ig_last_error()
    assert np.all(sc == -7)
    ok()
    # between ig_nuis_begin and ig_nuis_end the call refuses, and the step ends as if nothing had happened
    cands = s.return_neighbours(3, 5)
    p8 = np.array([float(s.param_simu[k][0]) for k in PARAM_NAMES], np.float32)
    s.ctx.nuis_begin(3, sorted(int(x) for x in cands if x != 3), p8, s.mean_kb())
    with pytest.raises(hip_lib.HipError, match="ig_placement_support.*in flight"):
        s.ctx.placement_support(64)
    with pytest.raises(hip_lib.HipError, match="in flight"):
        s.ctx.debug_placement_support_time(64)
    s.ctx.nuis_end()
    ok()
    with pytest.raises(ValueError):
        s.placement_support(window=8, window_kb=16.0)
    with pytest.raises(ValueError, match="min_hosts"):
        s.placement_support(window=8, min_hosts=17)
    s.free_gpu()
    # a sharded handle: the maximum needs the whole profile
    shard = problem_to_context(prob)
    shard.set_shard(0, 2)
    with pytest.raises(hip_lib.HipError, match="placement support needs all contacts on one handle"):
        shard.placement_support(64)
    shard.set_shard(0, 1)
    _assert_equal(shard.placement_support(64), ref, "whole again")
    shard.close()
    # before the contacts are uploaded, before a state
    bare = hip_lib.Context(0)
    bare.upload_subfrag_table(prob.np_sub_frags_2_frags)
    with pytest.raises(hip_lib.HipError, match="contacts"):
        bare.placement_support(64)
    bare.upload_contacts(prob.coo_row, prob.coo_col, prob.coo_cnt, prob.n_sub_frags)
    bare.set_insert_config(LIST_SIZE[:N_INSERT_BLOCKS], int(LIST_SIZE[:N_INSERT_BLOCKS].max() * np.int32(np.round(prob.S_o_A_frags["sub_len"].mean()) + 1)))
    with pytest.raises(hip_lib.HipError, match="state"):
        bare.placement_support(64)
    bare.upload_state(soa17_from_dict(prob.S_o_A_frags, prob.n_frags))
    _assert_equal(bare.placement_support(64), ref, "bare: no parameters needed")
    bare.close()


def test_nothing_placed_and_no_contacts():
    """T == 0 and Z == 0: success, no guest / no best site"""
    from instagraal_amd import hip_lib, placement_support as ps, synth
    from instagraal_amd.sampler import LIST_SIZE, N_INSERT_BLOCKS, problem_to_context, soa17_from_dict

    prob = synth.make_problem(*synth.CONFIGS["tiny"])
    ctx = problem_to_context(prob)
    for f in range(prob.n_frags):  # nothing placed: a bin of every contig is inactive
        ctx.debug_set_bin_active(f, False)
    for form in FORMS:
        ctx.debug_placement_support_form(form)
        got = ctx.placement_support(64)
        assert got["n_guests"] == 0 == got["n_contigs"] == got["entries"] and got["unplaced_observed"] == int(prob.coo_cnt.astype(np.int64).sum())
        assert np.all(got["status"] == 1) and all(np.all(got[k] == (-1 if k in ps.CONTIG_FIELDS else 0)) for k in ps.ARRAYS[1:])
    ctx.close()
    none = np.zeros(0, np.int32)  # no contacts at all
    bare = hip_lib.Context(0)
    bare.upload_subfrag_table(prob.np_sub_frags_2_frags)
    bare.upload_contacts(none, none, none, prob.n_sub_frags)
    bare.set_insert_config(LIST_SIZE[:N_INSERT_BLOCKS], int(LIST_SIZE[:N_INSERT_BLOCKS].max() * np.int32(np.round(prob.S_o_A_frags["sub_len"].mean()) + 1)))
    bare.upload_state(soa17_from_dict(prob.S_o_A_frags, prob.n_frags))
    t = _host_inputs(bare, prob)
    for form in FORMS:
        bare.debug_placement_support_form(form)
        got = bare.placement_support(64)
        _assert_equal(got, ps.support_host(*t, none, none, none, 64), ("no contacts", form))
        assert got["n_guests"] == prob.n_frags and not (got["best_contig"] >= 0).any() and (got["home_hosts"] > 0).all()
    bare.close()


def test_run_instagraal_save_placements_writes_one_file(tmp_path):
    from instagraal_amd import placement_support as ps, synth
    from instagraal_amd.simulation import run_instagraal

    data = str(tmp_path / "data")
    synth.write_text_dataset(data, n_contigs=10, mean_frags=110, seed=7, contacts_per_frag=40)
    np.random.seed(17)
    p2 = run_instagraal(data, os.path.join(data, "genome.fa"), output_folder=str(tmp_path / "out"), level=2, cycles=2, bomb=True, save_placements=True)
    folder = p2.simulation.output_folder
    s = p2.simulation.sampler
    assert [f for f in os.listdir(folder) if f.startswith("placements")] == ["placements.txt"]
    lines = open(os.path.join(folder, "placements.txt")).read().splitlines()
    assert lines[0][2:].split() == list(ps.PLACEMENT_COLUMNS)
    rows = [ln.split() for ln in lines if not ln.startswith("#")]
    sc = dict(kv.split("=") for kv in lines[-1][2:].split())
    res = s.placement_support()
    ranked = s.misplaced_bins(n=res["status"].size, result=res)
    assert len(rows) == ranked.size and [int(r[0]) for r in rows] == ranked["bin"].tolist() and int(sc["window"]) == 64 == int(sc["min_hosts"])
    upper = s.sparse_matrix.tocoo()
    total = int(upper.data[upper.row < upper.col].astype(np.int64).sum())  # what the device holds: the strict upper triangle
    assert sum(int(sc[k]) for k in ps.OBSERVED_SCALARS) == total and int(sc["n_guests"]) == res["n_guests"] > 0
    fasta = set(ln[1:].split()[0] for ln in open(os.path.join(folder, "genome.fasta")) if ln.startswith(">"))
    assert set(r[1] for r in rows) | set(r[5] for r in rows) <= fasta and all(float(r[10]) > 1.0 for r in rows)
    p2.simulation.release()
    data2 = str(tmp_path / "data2")  # (a folder of its own: the first run left its pyramid in the other)
    synth.write_text_dataset(data2, n_contigs=10, mean_frags=110, seed=7, contacts_per_frag=40)
    np.random.seed(17)
    p3 = run_instagraal(data2, os.path.join(data2, "genome.fa"), output_folder=str(tmp_path / "out2"), level=2, cycles=1, bomb=True)
    assert not [f for f in os.listdir(p3.simulation.output_folder) if f.startswith("placements")]
    p3.simulation.release()
