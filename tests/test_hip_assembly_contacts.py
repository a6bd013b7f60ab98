"""GPU tests of the contacts in the coordinates of the current genome (ig_assembly_contacts_build / _rows / _fetch,
sampler.assembly_contacts) against the rule's host statement (instagraal_amd.assembly_contacts.lift_host) on the order downloaded
from the same handle.  Every comparison is exact integer equality, most of them of the arrays' bytes."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FIXTURES = ("matrix_tiny_plain", "matrix_tiny_bomb")
LEVELS = ("sub", "bin")
ARRAYS = ("rowptr", "col", "count")


def _sampler(cfg, seed=None, coo=False, **extra):
    from instagraal_amd import synth
    from instagraal_amd.sampler import sampler as hip_sampler

    prob = synth.make_problem(*synth.CONFIGS[cfg])
    if seed is not None:
        np.random.seed(seed)
    kw = prob.sampler_kwargs()
    if coo is True:
        kw["coo"] = (prob.coo_row, prob.coo_col, prob.coo_cnt)
    elif coo is not False:
        kw["coo"] = coo
    kw.update(extra)
    s = hip_sampler(**kw, device_id=0)
    s.set_param_simu(dict(prob.params))
    s.bins = np.arange(1.0, 60.0, 1.0)
    s.eval_likelihood_init()
    return prob, s


def _host_inputs(ctx, prob):
    """what lift_host takes, from contact_map_order of the handle -> (order, position, unit of every position at level "bin")"""
    from instagraal_amd import assembly_contacts as ac

    order = ctx.contact_map_order().astype(np.int64)
    parent = prob.np_sub_frags_2_frags["x"].astype(np.int64)
    return order, ac.positions_of(order, prob.n_sub_frags), ac.units_along(parent[order])


def _rule(ctx, prob, level, contacts=None):
    from instagraal_amd import assembly_contacts as ac

    _, position, unit = _host_inputs(ctx, prob)
    row, col, cnt = contacts if contacts is not None else (prob.coo_row, prob.coo_col, prob.coo_cnt)
    return ac.lift_host(position, row, col, cnt, unit if level == "bin" else None)


def _device(ctx, level):
    """build + one fetch -> the rule's dict"""
    res = ctx.assembly_contacts(level)
    res["col"], res["count"] = ctx.assembly_contacts_fetch(0, res.pop("n_entries"))
    return res


def _assert_equal(got, want, what):
    from instagraal_amd import assembly_contacts as ac

    for k in ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (what, k)
    for k in ac.SCALARS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert got["contacts_kept"] == int(got["count"].sum()) and got["entries_out"] == got["col"].size


def _assert_device_equals_rule(s, prob, what, want_unplaced=False):
    total = int(prob.coo_cnt.astype(np.int64).sum())
    for level in LEVELS:
        want = _rule(s.ctx, prob, level)
        s.ctx.debug_assembly_contacts_combine(False)  # (one atomic per contact in the two passes: the same bytes)
        _assert_equal(_device(s.ctx, level), want, (what, level, "one atomic per contact"))
        s.ctx.debug_assembly_contacts_combine(True)
        got = _device(s.ctx, level)
        _assert_equal(got, want, (what, level))
        assert got["contacts_kept"] + got["contacts_unplaced"] == total and got["entries_in"] == prob.coo_cnt.size
        assert (got["entries_unplaced"] > 0) == want_unplaced, (what, level)
        if level == "sub":
            assert got["entries_out"] == got["entries_kept"]
    s.ctx.assembly_contacts_release()


@pytest.mark.parametrize("name", FIXTURES)
def test_device_equals_the_rule_on_the_fixture_states(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    prob, s = _sampler(str(g["config"]), seed=11)
    s.ctx.upload_state(g["state"])
    s.modify_gl_cuda_buffer()
    s.eval_likelihood_init()
    assert np.array_equal(s.ctx.contact_map_order(), g["full_order_high"])
    _assert_device_equals_rule(s, prob, name)
    s.free_gpu()


def test_device_equals_the_rule_on_small_fresh_after_moves_and_after_the_bomb():
    prob, s = _sampler("small", seed=12)
    _assert_device_equals_rule(s, prob, "small fresh")
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:300], 5)
    order = s.ctx.contact_map_order().astype(np.int64)
    assert np.any(np.diff(order) < 0)  # (positions are no longer monotone in the ids: min / max and flipped bins matter)
    _assert_device_equals_rule(s, prob, "small after batch moves")
    s.bomb_the_genome()
    _assert_device_equals_rule(s, prob, "small after the bomb")
    s.free_gpu()


def _first_and_last_of_a_contig(prob, min_frags=3):
    S = prob.S_o_A_frags
    ids, cnt = np.unique(S["id_c"], return_counts=True)
    c = ids[np.argmax(cnt >= min_frags)]
    fr = np.nonzero(S["id_c"] == c)[0]
    return int(fr[np.argmin(S["pos"][fr])]), int(fr[np.argmax(S["pos"][fr])])


def test_a_state_with_a_ring():
    prob, s = _sampler("small", seed=13)
    first, last = _first_and_last_of_a_contig(prob)
    s.test_copy_struct(first, last, 10)  # operator 10 on the two ends of one contig closes it on itself
    s.modify_gl_cuda_buffer()
    assert (s.gpu_vect_frags.copy_from_gpu().circ == 1).sum() >= 3
    _assert_device_equals_rule(s, prob, "small with a ring")
    s.free_gpu()


def test_a_state_with_an_unplaced_contig():
    """ig_upload_state refuses a state with an inactive bin, so the flag of one bin of a contig of several is cleared on the device
    (ig_debug_set_bin_active): the whole contig leaves the genome order and its contacts are counted as unplaced"""
    from instagraal_amd.hip_lib import FRAG_FIELDS

    prob, s = _sampler("small", seed=14)
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:100], 5)
    state = s.ctx.download_state()
    id_c = state[FRAG_FIELDS.index("id_c")]
    ids, n = np.unique(id_c, return_counts=True)
    members = np.nonzero(id_c == ids[np.argmax(n >= 3)])[0]
    s.ctx.debug_set_bin_active(members[1], False)
    assert s.ctx.download_state()[FRAG_FIELDS.index("activ")].tolist().count(0) == 1
    order = s.ctx.contact_map_order()
    parent = prob.np_sub_frags_2_frags["x"].astype(np.int64)
    assert order.size == prob.n_sub_frags - int(np.isin(parent, members).sum()) and not np.isin(parent[order], members).any()
    _assert_device_equals_rule(s, prob, "small with an unplaced contig", want_unplaced=True)
    s.ctx.debug_set_bin_active(members[1], True)
    _assert_device_equals_rule(s, prob, "small, the contig placed again")
    s.free_gpu()


def test_units_are_the_genome_order_and_the_levels_agree_with_the_contact_map():
    from instagraal_amd import assembly_contacts as ac, contact_map as cmap

    prob, s = _sampler("tiny", seed=15)
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:100], 5)
    g = s.gpu_vect_frags.copy_from_gpu()
    full_order = cmap.genome_order(g.pos, g.id_c, g.activ, g.id_d, g.ori, prob.np_sub_frags_id)[0]
    per_bin = s.assembly_contacts("bin", diagonal=False)
    assert per_bin["bins"]["bin"].tolist() == full_order and per_bin["n_units"] == len(full_order)
    sub = _device(s.ctx, "sub")
    T = sub["n_units"]
    image, b = s.ctx.contact_map(max(T, 1))
    assert b == 1 and image.shape == (T, T)
    D = np.zeros((T, T), np.int64)
    D[ac.rows_of(sub["rowptr"]), sub["col"]] = sub["count"]
    assert np.array_equal(D, np.triu(image, k=1)) and D.any()
    order, _, unit = _host_inputs(s.ctx, prob)
    U = per_bin["n_units"]
    B = np.zeros((U, U), np.int64)
    np.add.at(B, (unit[ac.rows_of(sub["rowptr"])], unit[sub["col"]]), sub["count"])
    i, j = np.nonzero(B)
    assert np.array_equal(ac.rows_of(per_bin["rowptr"]), i) and np.array_equal(per_bin["col"], j) and np.array_equal(per_bin["count"], B[i, j])
    assert np.any(i == j)  # (contacts between two sub-fragments of one bin are kept)
    s.free_gpu()


def _crafted_contacts(order):
    """contacts that give, by position under ``order``: three hub rows with an entry in every column to their right (two of them in
    one bin), rows of 1, 2, 63, 64 and 65 entries, and empty rows everywhere else -- more than one chunk of the reduction in all"""
    T = order.size
    pairs = []
    for hub in (6, 7, 100):
        pairs += [(hub, q) for q in range(hub + 1, T)]
    for p, n in ((200, 1), (210, 2), (300, 63), (400, 64), (500, 65)):
        pairs += [(p, p + 1 + k) for k in range(n)]
    pa, pb = np.array(pairs, np.int64).T
    a, b = order[pa], order[pb]
    row, col = np.minimum(a, b), np.maximum(a, b)
    by = np.lexsort((col, row))
    cnt = (1 + (np.arange(row.size) * 7919) % 50).astype(np.int32)
    return row[by].astype(np.int32), col[by].astype(np.int32), cnt, {6: T - 7, 7: T - 8, 100: T - 101, 200: 1, 210: 2, 300: 63, 400: 64, 500: 65}


def test_every_sort_form_and_every_boundary_between_them():
    from instagraal_amd import synth

    from instagraal_amd.sampler import problem_to_context

    prob0 = synth.make_problem(*synth.CONFIGS["tiny"])
    plain = problem_to_context(prob0)
    order0 = plain.contact_map_order().astype(np.int64)  # (the fresh genome's order does not depend on the contacts: checked below)
    plain.close()
    assert order0.size == prob0.n_sub_frags
    row, col, cnt, lengths = _crafted_contacts(order0)
    prob, s = _sampler("tiny", seed=16, coo=(row, col, cnt))
    assert np.array_equal(s.ctx.contact_map_order(), order0) and row.size > 2048  # (the reduction works in chunks of 2 048 entries: rows cross a chunk's end)
    hub = max(lengths.values())
    used = {k: 0 for k in ("short", "lds", "long")}
    for level in LEVELS:
        want = _rule(s.ctx, prob, level, (row, col, cnt))
        if level == "sub":
            got_lengths = np.diff(want["rowptr"])
            assert {int(p): int(got_lengths[p]) for p in np.nonzero(got_lengths)[0]} == lengths
        else:  # the hub rows hold runs of equal units, and the two hubs of one bin share a row
            assert want["entries_out"] < want["entries_kept"] and np.diff(want["rowptr"]).max() > hub // 4
        first = None
        for limits in ((0, 0), (4, 16), (64, 65), (1, 1), (hub, hub)):
            s.ctx.debug_assembly_contacts_limits(*limits)
            got = _device(s.ctx, level)
            _assert_equal(got, want, (level, limits))
            forms = s.ctx.debug_assembly_contacts_forms()
            for k in used:
                used[k] += forms[k][0]
            assert sum(forms[k][1] for k in used) <= want["entries_kept"]
            if limits == (1, 1):
                assert forms["short"][0] == forms["lds"][0] == 0 and forms["long"][0] > 0 and forms["runs"] == 0
            if limits == (4, 16):
                assert forms["runs"] > forms["long"][0] > 0 and forms["longest"] >= hub // 3
            if limits == (0, 0) and level == "sub":
                assert forms["short"] == (3, 2 + 63 + 64) and forms["lds"] == (4, 65 + sum(lengths[h] for h in (6, 7, 100))) and forms["long"][0] == 0
            blob = b"".join(got[k].tobytes() for k in ARRAYS)
            first = blob if first is None else first
            assert blob == first
    assert all(v > 0 for v in used.values()), used
    s.ctx.debug_assembly_contacts_limits(0, 0)
    s.ctx.debug_assembly_contacts_combine(False)
    _assert_equal(_device(s.ctx, "bin"), want, "one atomic per contact")
    s.ctx.debug_assembly_contacts_combine(True)
    s.ctx.debug_assembly_contacts_limits(0, 0)
    with pytest.raises(Exception, match="limit"):
        s.ctx.debug_assembly_contacts_limits(-1, 0)
    s.free_gpu()


def test_cfg2_takes_the_long_form_at_the_default_caps_and_the_scans_carry_loop():
    """5 000 bins, 14 900 sub-fragments, 2 000 000 contacts under the limits the library ships: more than 256 chunks of entries, so the
    reduction's scan of the heads takes its carry loop twice, and, at bin level, rows longer than the 1 024 entries of the lds form:
    the long form with whole runs, merge widths from 1 024 up and the copy-back step.
    Which states have such rows is the data's business, so the rule says it and the device is held to the rule: the genome order
    puts the contigs by their canonical ids (by length), not by bin number, and under it the longest raw row at bin level measures
    1 000 on the fresh genome and 947 after 1 000 batch moves (34 rows of up to 1 085 under the order of the bin numbers); with every
    bin a contig of its own it measures 1 071, with 30 rows beyond 1 024.  So the genome is bombed as a third state, and there the
    long form must have run."""
    import test_rows_rule_host as rule

    prob, s = _sampler("cfg2", seed=21)
    long_rows_seen = {}
    try:
        for state in ("fresh", "after batch moves", "bombed"):
            if state == "after batch moves":
                s.step_sampler_batch(np.random.permutation(prob.n_frags)[:1000], 5)
            if state == "bombed":
                s.bomb_the_genome()
            _, position, unit = _host_inputs(s.ctx, prob)
            for level in LEVELS:
                want = _rule(s.ctx, prob, level)
                key = position if level == "sub" else np.where(position >= 0, unit[np.maximum(position, 0)], -1)
                a, b = key[prob.coo_row], key[prob.coo_col]
                lengths = np.bincount(np.minimum(a, b)[(a >= 0) & (b >= 0)], minlength=want["n_units"])  # the rows before the reduction
                assert int(lengths.sum()) == want["entries_kept"] > 256 * rule.SCAN_CHUNK
                long_rows = lengths > rule.LDS_CAP
                long_rows_seen[state, level] = int(long_rows.sum())
                for combine in (False, True):
                    s.ctx.debug_assembly_contacts_combine(combine)
                    _assert_equal(_device(s.ctx, level), want, (state, level, combine))
                    forms = s.ctx.debug_assembly_contacts_forms()
                    print(state, level, "combine" if combine else "one atomic per contact", "longest raw row", int(lengths.max()), forms)
                    assert forms == rule.forms_rule(lengths, (0, 0)), (state, level, combine)
                    assert forms["long"] == (int(long_rows.sum()), int(lengths[long_rows].sum())), (state, level, combine)
        assert long_rows_seen["bombed", "bin"] > 0, long_rows_seen  # (the forms above equal the rule's: the long form ran there)
    finally:
        s.ctx.debug_assembly_contacts_combine(True)
        s.ctx.assembly_contacts_release()
        s.free_gpu()


def test_two_builds_agree_fetches_in_pieces_and_the_snapshot():
    from instagraal_amd import hip_lib

    prob, s = _sampler("tiny", seed=17)
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:100], 5)
    for level in LEVELS:
        a = _device(s.ctx, level)
        b = _device(s.ctx, level)
        for k in ARRAYS:
            assert a[k].tobytes() == b[k].tobytes()
        n = a["entries_out"]
        for step in (1, 1000, 997):
            parts = [s.ctx.assembly_contacts_fetch(o, min(step, n - o)) for o in range(0, n, step)]
            assert np.array_equal(np.concatenate([p[0] for p in parts]), a["col"]) and np.array_equal(np.concatenate([p[1] for p in parts]), a["count"])
        assert s.ctx.assembly_contacts_fetch(n, 0)[0].size == 0
    before = s.ctx.contact_map_order()
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:50], 5)
    assert not np.array_equal(s.ctx.contact_map_order(), before)  # the genome moved on, the snapshot did not
    col, count = s.ctx.assembly_contacts_fetch(0, a["entries_out"])
    assert np.array_equal(col, a["col"]) and np.array_equal(count, a["count"])
    s.ctx.assembly_contacts_release()
    with pytest.raises(hip_lib.HipError, match="nothing is built"):
        s.ctx.assembly_contacts_fetch(0, 1)
    s.ctx.assembly_contacts_release()  # (twice is fine)
    s.free_gpu()


def test_the_pass_disturbs_nothing():
    outs = []
    for with_build in (False, True):
        prob, s = _sampler("small", seed=3)
        frags = np.random.permutation(prob.n_frags)[:200]
        res = [s.step_sampler_batch(frags[:100], 5)]
        if with_build:
            for level in LEVELS:
                assert _device(s.ctx, level)["entries_out"] > 0
            ms, _ = s.ctx.debug_assembly_contacts_time("bin", n=2)
            assert ms.shape == (2, 7) and (ms[:, :3] > 0).all()
            assert s.assembly_contacts("sub")["count"].sum() > 0
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


def test_the_shards_merge_to_the_whole():
    from instagraal_amd import assembly_contacts as ac, synth
    from instagraal_amd.sampler import problem_to_context

    prob = synth.make_problem(*synth.CONFIGS["small"])
    whole = problem_to_context(prob)
    shards = []
    for rank in range(2):
        ctx = problem_to_context(prob)
        ctx.set_shard(rank, 2)
        shards.append(ctx)
    for level in LEVELS:
        want = _device(whole, level)
        parts = [_device(ctx, level) for ctx in shards]
        assert all(p["entries_out"] > 0 for p in parts)
        U = want["n_units"]
        key = np.concatenate([ac.rows_of(p["rowptr"]) * U + p["col"] for p in parts])
        val = np.concatenate([p["count"] for p in parts])
        keys, inverse = np.unique(key, return_inverse=True)
        count = np.zeros(keys.size, np.int64)
        np.add.at(count, inverse, val)
        assert np.array_equal(keys, ac.rows_of(want["rowptr"]) * U + want["col"]) and np.array_equal(count, want["count"])
        for k in ac.SUMMED_SCALARS:
            assert parts[0][k] + parts[1][k] == want[k], (level, k)
        for k in ("n_placed", "n_units"):
            assert parts[0][k] == parts[1][k] == want[k]
        if level == "sub":  # (a row lives on one rank: no key is shared)
            assert parts[0]["entries_out"] + parts[1]["entries_out"] == want["entries_out"] == keys.size == key.size
    for ctx in shards + [whole]:
        ctx.close()


def test_errors_are_loud_and_leave_the_context_usable():
    from instagraal_amd import hip_lib
    from instagraal_amd.sampler import LIST_SIZE, N_INSERT_BLOCKS, PARAM_NAMES, soa17_from_dict

    prob, s = _sampler("tiny")
    ref = _device(s.ctx, "sub")

    def ok():
        got = _device(s.ctx, "sub")
        assert all(got[k].tobytes() == ref[k].tobytes() for k in ARRAYS)

    for bad in (2, -1):
        with pytest.raises(hip_lib.HipError, match="level"):
            s.ctx.assembly_contacts(bad)
        with pytest.raises(hip_lib.HipError, match="nothing is built"):  # (a failed build leaves no stale result)
            s.ctx.assembly_contacts_fetch(0, 1)
        ok()
    n = ref["entries_out"]
    for first, count in ((n, 1), (-1, 1), (0, n + 1), (0, -1), (n + 1, 0)):
        with pytest.raises(hip_lib.HipError, match="out of range"):
            s.ctx.assembly_contacts_fetch(first, count)
    assert np.array_equal(s.ctx.assembly_contacts_fetch(0, n)[0], ref["col"])
    lib = hip_lib.lib()
    rows = np.full(ref["n_units"] + 1, -7, np.int64)
    assert lib.ig_assembly_contacts_rows(s.ctx._h, C.c_void_p(rows.ctypes.data), C.c_int64(ref["n_units"])) != 0
    assert b"capacity" in lib.ig_last_error() and np.all(rows == -7)
    assert lib.ig_assembly_contacts_rows(s.ctx._h, C.c_void_p(rows.ctypes.data), C.c_int64(rows.size)) == 0 and np.array_equal(rows, ref["rowptr"])
    ok()
    # between ig_nuis_begin and ig_nuis_end the build refuses, and the step ends as if nothing had happened
    cands = s.return_neighbours(3, 5)
    p8 = np.array([float(s.param_simu[k][0]) for k in PARAM_NAMES], np.float32)
    s.ctx.nuis_begin(3, sorted(int(x) for x in cands if x != 3), p8, s.mean_kb())
    with pytest.raises(hip_lib.HipError, match="ig_assembly_contacts_build.*in flight"):
        s.ctx.assembly_contacts("sub")
    with pytest.raises(hip_lib.HipError, match="in flight"):
        s.ctx.debug_assembly_contacts_time("sub")
    s.ctx.nuis_end()
    assert _device(s.ctx, "bin")["entries_out"] > 0
    s.free_gpu()
    # before the contacts are uploaded
    bare = hip_lib.Context(0)
    bare.upload_subfrag_table(prob.np_sub_frags_2_frags)
    with pytest.raises(hip_lib.HipError, match="contacts"):
        bare.assembly_contacts("sub")
    bare.upload_contacts(prob.coo_row, prob.coo_col, prob.coo_cnt, prob.n_sub_frags)
    bare.set_insert_config(LIST_SIZE[:N_INSERT_BLOCKS], int(LIST_SIZE[:N_INSERT_BLOCKS].max() * np.int32(np.round(prob.S_o_A_frags["sub_len"].mean()) + 1)))
    with pytest.raises(hip_lib.HipError, match="state"):
        bare.assembly_contacts("sub")
    bare.upload_state(soa17_from_dict(prob.S_o_A_frags, prob.n_frags))
    got = _device(bare, "sub")
    assert all(got[k].tobytes() == ref[k].tobytes() for k in ARRAYS)
    bare.upload_contacts(prob.coo_row, prob.coo_col, prob.coo_cnt, prob.n_sub_frags)  # a new upload releases the result
    with pytest.raises(hip_lib.HipError, match="nothing is built"):
        bare.assembly_contacts_fetch(0, 1)
    bare.close()


def test_sampler_assembly_contacts_with_the_diagonal():
    import scipy.sparse as sp

    from instagraal_amd import assembly_contacts as ac, synth

    prob0 = synth.make_problem(*synth.CONFIGS["tiny"])
    M = prob0.n_sub_frags
    d = np.zeros(M, np.int32)
    d[::5] = 1 + np.arange(M)[::5] % 9
    prob, s = _sampler("tiny", seed=18, sparse_matrix=(prob0.sub_csr + sp.diags(d, format="csr")).tocsr())
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:100], 5)
    order, position, unit = _host_inputs(s.ctx, prob)
    sym_d = np.asarray(s.sparse_matrix.diagonal()).astype(np.int64)
    assert sym_d.sum() == 2 * int(d.sum()) > 0
    for level in LEVELS:
        want = _rule(s.ctx, prob, level)
        U = want["n_units"]
        D = np.zeros((U, U), np.int64)
        D[ac.rows_of(want["rowptr"]), want["col"]] = want["count"]
        u = np.arange(order.size) if level == "sub" else unit
        np.add.at(D, (u, u), sym_d[order])
        i, j = np.nonzero(D)
        got = s.assembly_contacts(level)
        assert np.array_equal(ac.rows_of(got["rowptr"]), i) and np.array_equal(got["col"], j) and np.array_equal(got["count"], D[i, j])
        assert got["contacts_diagonal"] == int(sym_d[order].sum()) and got["count"].sum() == got["contacts_kept"] + got["contacts_diagonal"]
        for k in ac.SCALARS:  # the scalars describe the device's result
            assert got[k] == want[k], (level, k)
        assert np.array_equal(got["order"], order) and got["bins"].size == U
        ids, sizes = got["chrom_sizes"]
        assert int(sizes.sum()) == int(prob.S_o_A_sub_frags["len_bp"][order].astype(np.int64).sum())
        lean = s.assembly_contacts(level, diagonal=False)
        assert all(lean[k].tobytes() == want[k].tobytes() for k in ARRAYS) and lean["contacts_diagonal"] == 0
    s.free_gpu()


def test_write_assembly_contacts_on_small_after_moves(tmp_path):
    from instagraal_amd import assembly_contacts as ac

    prob, s = _sampler("small", seed=19)
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:300], 5)
    for level in LEVELS:
        want = s.assembly_contacts(level)
        folder = str(tmp_path / level)
        sc = s.write_assembly_contacts(folder, level=level, block_rows=257)
        assert all(sc[k] == want[k] for k in ac.SCALARS) and sc["pixels_written"] == want["col"].size
        px = np.loadtxt(os.path.join(folder, "pixels.tsv"), dtype=np.int64, ndmin=2)
        assert np.array_equal(px[:, 0], ac.rows_of(want["rowptr"])) and np.array_equal(px[:, 1], want["col"]) and np.array_equal(px[:, 2], want["count"])
        bed = np.loadtxt(os.path.join(folder, "bins.bed"), dtype=str, ndmin=2)
        assert bed[:, 0].tolist() == ac.scaffold_names(want["bins"]["contig"]).tolist()
        assert np.array_equal(bed[:, 1].astype(np.int64), want["bins"]["start"]) and np.array_equal(bed[:, 2].astype(np.int64), want["bins"]["end"])
        sizes = np.loadtxt(os.path.join(folder, "chrom.sizes"), dtype=str, ndmin=2)
        assert np.array_equal(sizes[:, 1].astype(np.int64), want["chrom_sizes"][1])
    s.free_gpu()


def test_run_instagraal_save_contacts_writes_the_three_files_once(tmp_path):
    from instagraal_amd import assembly_contacts as ac, synth
    from instagraal_amd.simulation import run_instagraal

    data = str(tmp_path / "data")
    synth.write_text_dataset(data, n_contigs=10, mean_frags=110, seed=7, contacts_per_frag=40)
    np.random.seed(17)
    p2 = run_instagraal(data, os.path.join(data, "genome.fa"), output_folder=str(tmp_path / "out"), level=2, cycles=2, bomb=True, save_contacts=True)
    folder = p2.simulation.output_folder
    s = p2.simulation.sampler
    out = os.path.join(folder, "assembly_contacts")
    assert sorted(os.listdir(out)) == ["bins.bed", "chrom.sizes", "pixels.tsv"]
    assert not [f for f in os.listdir(folder) if f.startswith("assembly_contacts_")]  # (once, not per cycle)
    g = s.gpu_vect_frags.copy_from_gpu()
    parent = s.np_sub_frags_2_frags["x"].astype(np.int64)
    order = s.ctx.contact_map_order().astype(np.int64)
    len_bp = np.asarray(s.S_o_A_sub_frags["len_bp"]).astype(np.int64)
    contig = g.id_c.astype(np.int64)[parent[order]]
    want = {ac.SCAFFOLD_PREFIX + str(c): int(len_bp[order][contig == c].sum()) for c in np.unique(contig)}
    sizes = dict((ln.split("\t")[0], int(ln.split("\t")[1])) for ln in open(os.path.join(out, "chrom.sizes")).read().splitlines())
    assert sizes == want
    fasta, name = {}, None
    for ln in open(os.path.join(folder, "genome.fasta")):
        if ln.startswith(">"):
            name = ln[1:].strip()
            fasta[name] = 0
        else:
            fasta[name] += len(ln.strip())
    assert set(fasta) == set(sizes)
    for k in sorted(sizes):  # (not asserted: the pyramid's kept quirks may move the lengths)
        print("%s chrom.sizes %d genome.fasta %d" % (k, sizes[k], fasta[k]))
    px = np.loadtxt(os.path.join(out, "pixels.tsv"), dtype=np.int64, ndmin=2)
    U = order.size
    assert px.shape[0] > 0 and np.all(px[:, 0] <= px[:, 1]) and px[:, 1].max() < U and np.all(np.diff(px[:, 0] * U + px[:, 1]) > 0)
    assert len(open(os.path.join(out, "bins.bed")).read().splitlines()) == U
    upper = s.sparse_matrix.tocoo()  # (symmetrised: its upper triangle with the diagonal is what the file holds, between placed ends)
    position = ac.positions_of(order, parent.size)
    keep = (upper.row <= upper.col) & (position[upper.row] >= 0) & (position[upper.col] >= 0)
    assert int(px[:, 2].sum()) == int(upper.data[keep].astype(np.int64).sum())
    p2.simulation.release()
    data2 = str(tmp_path / "data2")  # (a folder of its own: the first run left its pyramid in the other)
    synth.write_text_dataset(data2, n_contigs=10, mean_frags=110, seed=7, contacts_per_frag=40)
    np.random.seed(17)
    p3 = run_instagraal(data2, os.path.join(data2, "genome.fa"), output_folder=str(tmp_path / "out2"), level=2, cycles=1, bomb=True)
    assert not os.path.exists(os.path.join(p3.simulation.output_folder, "assembly_contacts"))
    p3.simulation.release()
