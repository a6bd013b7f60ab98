"""GPU tests of the fixed-resolution maps (ig_assembly_contacts_build_units, ig_assembly_contacts_coarsen, ig_balance_build_units,
sampler.resolution_contacts / scaffold_contacts / write_zoom_levels) against the rule's host statement
(instagraal_amd.zoom_levels) on the order downloaded from the same handle.  Every comparison is exact integer equality, most of
them of the arrays' bytes."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

BINSIZES = (889, 3556, 12446)  # `small`: about half the median sub-fragment length, 2 x and 7 x that
FACTORS = (2, 3, 5)
ARRAYS = ("rowptr", "col", "count")
CARRIED = ("contacts_kept", "entries_unplaced", "contacts_unplaced", "n_placed", "n_units", "entries_out")
LIMITS = ((0, 0), (4, 16), (64, 65), (1, 1), (3000, 3000))  # the settings of test_hip_assembly_contacts.py (its hub: the longest segment here)


def _sampler(cfg, seed=None, **extra):
    import test_hip_assembly_contacts as ta

    return ta._sampler(cfg, seed, **extra)


class Frame:
    """the host's view of a handle's current genome: the order, the positions, the sub-fragment table, the scaffold sizes"""

    def __init__(self, ctx, prob):
        from instagraal_amd import assembly_contacts as ac
        from instagraal_amd.hip_lib import FRAG_FIELDS

        self.prob = prob
        self.order = ctx.contact_map_order().astype(np.int64)
        self.position = ac.positions_of(self.order, prob.n_sub_frags)
        self.parent = prob.np_sub_frags_2_frags["x"].astype(np.int64)
        st = ctx.download_state()
        self.table = ac.bins_table(self.order, self.parent, st[FRAG_FIELDS.index("id_c")].astype(np.int64), st[FRAG_FIELDS.index("ori")].astype(np.int64),
                                   prob.S_o_A_sub_frags["len_bp"], "sub")
        self.sizes = ac.chrom_sizes(self.table)

    def units(self, what):
        from instagraal_amd import zoom_levels as zl

        return zl.scaffold_units(self.table) if what == "scaffold" else zl.units_of_positions(self.table, what)

    def rule(self, unit, U, contacts=None):
        from instagraal_amd import zoom_levels as zl

        row, col, cnt = contacts if contacts is not None else (self.prob.coo_row, self.prob.coo_col, self.prob.coo_cnt)
        return zl.lift_units_host(self.position, row, col, cnt, unit, U)


def _fetched(ctx, res):
    res["col"], res["count"] = ctx.assembly_contacts_fetch(0, res.pop("n_entries"))
    return res


def _built(ctx, unit, U):
    return _fetched(ctx, ctx.assembly_contacts_units(unit, U))


def _coarsened(ctx, m, C_):
    return _fetched(ctx, ctx.assembly_contacts_coarsen(m, C_))


def _assert_equal(got, want, what, scalars=None):
    from instagraal_amd import assembly_contacts as ac

    for k in ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (what, k)
    for k in ac.SCALARS if scalars is None else scalars:
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert got["contacts_kept"] == int(got["count"].sum()) and got["entries_out"] == got["col"].size == got["rowptr"][-1]


def _assert_state(s, prob, what, want_unplaced=False):
    """the units build in both combine forms and every coarsening of the issue's list against the rule, on the handle's genome"""
    from instagraal_amd import assembly_contacts as ac, zoom_levels as zl

    fr = Frame(s.ctx, prob)
    direct = {}
    for B in BINSIZES + ("scaffold",):
        unit, U = fr.units(B)
        want = direct[B] = fr.rule(unit, U)
        s.ctx.debug_assembly_contacts_combine(False)
        _assert_equal(_built(s.ctx, unit, U), want, (what, B, "one atomic per contact"))
        s.ctx.debug_assembly_contacts_combine(True)
        got = _built(s.ctx, unit, U)
        _assert_equal(got, want, (what, B))
        assert (got["entries_unplaced"] > 0) == want_unplaced and got["n_units"] == U and got["n_placed"] == fr.order.size
    # with the table of level "bin" the result is ig_assembly_contacts_build(level = 1), byte for byte
    unit = ac.units_along(fr.parent[fr.order])
    per_bin = _fetched(s.ctx, s.ctx.assembly_contacts("bin"))
    per_bin.pop("level")
    _assert_equal(_built(s.ctx, unit, int(unit[-1]) + 1 if unit.size else 0), per_bin, (what, "the bins' own table"))
    # coarsening a built level is building the coarser one
    for B in BINSIZES:
        unit, U = fr.units(B)
        for f in FACTORS:
            unit_c, U_c = fr.units(f * B)
            want = fr.rule(unit_c, U_c)
            _built(s.ctx, unit, U)
            got = _coarsened(s.ctx, *zl.coarse_map(fr.sizes, B, f))
            _assert_equal(got, want, (what, B, f), CARRIED)
            assert got["entries_in"] == got["entries_kept"] == direct[B]["entries_out"]
        # the chain x2, x5 against x10; then on to the scaffolds
        _built(s.ctx, unit, U)
        s.ctx.assembly_contacts_coarsen(*zl.coarse_map(fr.sizes, B, 2))
        got = _coarsened(s.ctx, *zl.coarse_map(fr.sizes, 2 * B, 5))
        _assert_equal(got, fr.rule(*fr.units(10 * B)), (what, B, "x2 x5"), CARRIED)
        _assert_equal(_coarsened(s.ctx, *zl.scaffold_map(fr.sizes, 10 * B)), direct["scaffold"], (what, B, "to the scaffolds"), CARRIED)
    # the identity map returns its input, one coarse unit the one pixel with the total
    unit, U = fr.units(BINSIZES[1])
    _built(s.ctx, unit, U)
    _assert_equal(_coarsened(s.ctx, np.arange(U), U), direct[BINSIZES[1]], (what, "identity"), CARRIED)
    got = _coarsened(s.ctx, np.zeros(U, np.int64), 1)
    kept = direct[BINSIZES[1]]["contacts_kept"]
    assert got["rowptr"].tolist() == ([0, 1] if kept else [0, 0]) and got["col"].tolist() == [0] * bool(kept) and got["count"].tolist() == [kept] * bool(kept)
    s.ctx.assembly_contacts_release()
    return direct


@pytest.mark.parametrize("name", ("matrix_tiny_plain", "matrix_tiny_bomb"))
def test_the_fixture_states(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    prob, s = _sampler(str(g["config"]), seed=11)
    s.ctx.upload_state(g["state"])
    s.modify_gl_cuda_buffer()
    s.eval_likelihood_init()
    assert np.array_equal(s.ctx.contact_map_order(), g["full_order_high"])
    _assert_state(s, prob, name)
    s.free_gpu()


def test_small_fresh_after_moves_and_after_the_bomb():
    from instagraal_amd import zoom_levels as zl

    prob, s = _sampler("small", seed=12)
    direct = _assert_state(s, prob, "small fresh")
    fr = Frame(s.ctx, prob)
    gaps = [zl.units_without_position(*fr.units(B)) for B in BINSIZES]
    assert gaps[0] > 0 and gaps[2] == 0, gaps  # a resolution below what the fragments carry has empty rows; 7 x above it has none
    assert direct[BINSIZES[0]]["n_units"] > fr.order.size  # more units than positions at the first bin size
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:300], 5)
    assert np.any(np.diff(s.ctx.contact_map_order().astype(np.int64)) < 0)
    _assert_state(s, prob, "small after batch moves")
    s.bomb_the_genome()
    _assert_state(s, prob, "small after the bomb")
    s.free_gpu()


def test_a_state_with_a_ring_and_one_with_an_unplaced_contig():
    import test_hip_assembly_contacts as ta
    from instagraal_amd.hip_lib import FRAG_FIELDS

    prob, s = _sampler("small", seed=13)
    first, last = ta._first_and_last_of_a_contig(prob)
    s.test_copy_struct(first, last, 10)
    s.modify_gl_cuda_buffer()
    assert (s.gpu_vect_frags.copy_from_gpu().circ == 1).sum() >= 3
    _assert_state(s, prob, "small with a ring")
    s.free_gpu()
    prob, s = _sampler("small", seed=14)
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:100], 5)
    id_c = s.ctx.download_state()[FRAG_FIELDS.index("id_c")]
    ids, n = np.unique(id_c, return_counts=True)
    members = np.nonzero(id_c == ids[np.argmax(n >= 3)])[0]
    s.ctx.debug_set_bin_active(members[1], False)
    assert s.ctx.contact_map_order().size < prob.n_sub_frags
    _assert_state(s, prob, "small with an unplaced contig", want_unplaced=True)
    s.free_gpu()


# ---- the coarsening over crafted CSR data (ig_debug_zoom_coarsen)

def test_the_coarsening_over_crafted_rows_under_every_limit():
    import test_rows_rule_host as rule
    import test_zoom_levels_host as zh
    from instagraal_amd import hip_lib, zoom_levels as zl

    ctx = hip_lib.Context(0)  # a bare handle: nothing uploaded
    used = {k: 0 for k in ("short", "lds", "long")}
    for name, (rowptr, col, count, m, C_) in (("cases", zh.crafted()[:5]), ("spread", zh.crafted_spread())):
        want = zl.coarsen_host(rowptr, col, count, m, C_)
        lengths = np.bincount(m[np.repeat(np.arange(m.size), np.diff(rowptr))], minlength=C_)  # the raw segments
        if name == "spread":
            assert int(want[2].max()) > 2 ** 32 and np.diff(want[0]).max() > 64 and lengths.max() > rule.LDS_CAP
        for limits in LIMITS:
            ctx.debug_assembly_contacts_limits(*limits)
            got = ctx.debug_zoom_coarsen(rowptr, col, count, m, C_)
            for g, w, k in zip((got["rowptr"], got["col"], got["count"]), want, ARRAYS):
                assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (name, limits, k)
            assert got["n_out"] == want[1].size
            assert got["forms"] == rule.forms_rule(lengths, limits), (name, limits)
            for k in used:
                used[k] += got["forms"][k][0]
            if name == "cases" and limits == (0, 0):
                assert got["forms"]["short"] == (6, 2 + 63 + 64 + 5 + 3 + 3) and got["forms"]["lds"] == (2, 65 + 1024) and got["forms"]["long"] == (2, 1025 + 3000)
    assert all(v > 0 for v in used.values()), used
    ctx.debug_assembly_contacts_limits(0, 0)
    # an empty level, and a level without rows
    got = ctx.debug_zoom_coarsen(np.zeros(4, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int64), [0, 0, 1], 3)
    assert got["rowptr"].tolist() == [0, 0, 0, 0] and got["n_out"] == 0
    got = ctx.debug_zoom_coarsen(np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(0, np.int64), 0)
    assert got["rowptr"].tolist() == [0] and got["n_out"] == 0
    for bad, words in ((dict(m=[1, 0, 1]), "not monotone"), (dict(m=[0, 1, 3]), "out of range"), (dict(col=[5]), "column"), (dict(rowptr=[0, 1, 0, 1]), "decreases")):
        a = dict(rowptr=[0, 1, 1, 1], col=[2], count=[7], m=[0, 1, 2])
        a.update(bad)
        with pytest.raises(hip_lib.HipError, match=words):
            ctx.debug_zoom_coarsen(a["rowptr"], a["col"], a["count"], a["m"], 3)
    ctx.close()


# ---- large counts, shards, refusals, the snapshot


@pytest.mark.parametrize("family", ("narrow_max", "wide_min", "int_max"))
def test_large_counts(family):
    """the inputs of tests/_large_counts.py on both sides of their thresholds: the units build and a coarsening against the rule, the
    totals in Python integers"""
    import _large_counts as lc
    import test_hip_large_counts as tl
    from instagraal_amd import zoom_levels as zl

    prob = tl._prob(family)
    s = tl._sampler_of(prob, seed=23)
    fr = Frame(s.ctx, prob)
    B = BINSIZES[1]
    unit, U = fr.units(B)
    want = fr.rule(unit, U)
    got = _built(s.ctx, unit, U)
    _assert_equal(got, want, family)
    assert sum(got["count"].tolist()) + got["contacts_unplaced"] == tl._total(prob)
    got = _coarsened(s.ctx, *zl.coarse_map(fr.sizes, B, 5))
    _assert_equal(got, fr.rule(*fr.units(5 * B)), (family, "x5"), CARRIED)
    assert sum(got["count"].tolist()) == sum(want["count"].tolist())
    if family == "int_max":
        assert got["count"].max() > 2 ** 32
    got = _coarsened(s.ctx, *zl.scaffold_map(fr.sizes, 5 * B))
    _assert_equal(got, fr.rule(*fr.units("scaffold")), (family, "scaffolds"), CARRIED)
    assert lc.INT_MAX < got["count"].max() or family != "int_max"
    s.ctx.assembly_contacts_release()
    s.free_gpu()


def test_two_shards_merge_to_the_whole():
    from instagraal_amd import assembly_contacts as ac, synth, zoom_levels as zl
    from instagraal_amd.sampler import problem_to_context

    prob = synth.make_problem(*synth.CONFIGS["small"])
    whole = problem_to_context(prob)
    shards = []
    for rank in range(2):
        ctx = problem_to_context(prob)
        ctx.set_shard(rank, 2)
        shards.append(ctx)
    fr = Frame(whole, prob)
    B = BINSIZES[1]
    unit, U = fr.units(B)

    def merged(parts, n):
        key = np.concatenate([ac.rows_of(p["rowptr"]) * n + p["col"] for p in parts])
        keys, inverse = np.unique(key, return_inverse=True)
        count = np.zeros(keys.size, np.int64)
        np.add.at(count, inverse.ravel(), np.concatenate([p["count"] for p in parts]))
        return keys, count

    for step in ("units", "coarsen"):
        if step == "units":
            want, parts, n = _built(whole, unit, U), [_built(ctx, unit, U) for ctx in shards], U
        else:
            m, n = zl.coarse_map(fr.sizes, B, 3)
            want, parts = _coarsened(whole, m, n), [_coarsened(ctx, m, n) for ctx in shards]
        assert all(p["entries_out"] > 0 for p in parts)
        keys, count = merged(parts, n)
        assert np.array_equal(keys, ac.rows_of(want["rowptr"]) * n + want["col"]) and np.array_equal(count, want["count"])
        for k in ("contacts_kept", "entries_unplaced", "contacts_unplaced"):
            assert parts[0][k] + parts[1][k] == want[k], (step, k)
        assert parts[0]["n_units"] == parts[1]["n_units"] == want["n_units"] == n
    for ctx in shards + [whole]:
        ctx.close()


def test_refusals_leave_nothing_built_and_the_handle_usable():
    from instagraal_amd import hip_lib, zoom_levels as zl

    prob, s = _sampler("tiny", seed=31)
    fr = Frame(s.ctx, prob)
    B = 3528
    unit, U = fr.units(B)
    want = fr.rule(unit, U)
    lib = hip_lib.lib()
    T = unit.size

    def nothing_built():
        with pytest.raises(hip_lib.HipError, match="nothing is built"):
            s.ctx.assembly_contacts_fetch(0, 1)

    def works():
        _assert_equal(_built(s.ctx, unit, U), want, "the next build")

    def raw_build(tab, n_pos, n_units):
        """the C entry itself, with outputs that must stay untouched"""
        t = np.ascontiguousarray(tab, np.int32)
        ne, sc = C.c_int64(-7), np.full(8, -7, np.int64)
        rc = lib.ig_assembly_contacts_build_units(s.ctx._h, C.c_void_p(t.ctypes.data), C.c_int64(n_pos), C.c_int64(n_units), C.byref(ne), C.c_void_p(sc.ctypes.data))
        assert rc != 0 and ne.value == -7 and np.all(sc == -7)
        return lib.ig_last_error().decode()

    bad = unit.copy()
    bad[5], bad[6] = unit[6] + 1, unit[5]
    for tab, n_pos, n_units, words in ((bad, T, U, "not monotone"), (np.where(np.arange(T) == T - 1, U, unit), T, U, "out of range"),
                                       (np.where(np.arange(T) == 0, -1, unit), T, U, "out of range"), (unit[:-1], T - 1, U, "positions"),
                                       (unit, T, 1 << 31, "2\\^31")):
        works()
        assert __import__("re").search(words, raw_build(tab, n_pos, n_units)), words
        nothing_built()
    works()

    def raw_coarsen(m, n_units, n_coarse):
        t = np.ascontiguousarray(m, np.int32)
        ne, sc = C.c_int64(-7), np.full(8, -7, np.int64)
        rc = lib.ig_assembly_contacts_coarsen(s.ctx._h, C.c_void_p(t.ctypes.data), C.c_int64(n_units), C.c_int64(n_coarse), C.byref(ne), C.c_void_p(sc.ctypes.data))
        assert rc != 0 and ne.value == -7 and np.all(sc == -7)
        return lib.ig_last_error().decode()

    m, C_ = zl.coarse_map(fr.sizes, B, 2)
    s.ctx.assembly_contacts_release()
    assert "nothing is built" in raw_coarsen(m, U, C_)
    s.ctx.assembly_contacts("sub")
    assert "level 0" in raw_coarsen(np.arange(T), T, T)
    nothing_built()
    rev = m.copy()
    rev[3], rev[4] = m[-1], m[0]
    for mm, n_u, n_c, words in ((m, U - 1, C_, "units"), (rev, U, C_, "not monotone"), (np.where(np.arange(U) == U - 1, C_, m), U, C_, "out of range"),
                                (m, U, 1 << 31, "2\\^31")):
        works()
        assert __import__("re").search(words, raw_coarsen(mm, n_u, n_c)), words
        nothing_built()  # a failed coarsening leaves nothing to fetch
    works()
    got = _coarsened(s.ctx, m, C_)
    _assert_equal(got, fr.rule(*fr.units(2 * B)), "behind the refusals", CARRIED)
    s.ctx.assembly_contacts_release()
    s.free_gpu()


def test_fetches_in_pieces_and_the_snapshot_stays_while_the_genome_moves():
    from instagraal_amd import zoom_levels as zl

    prob, s = _sampler("tiny", seed=17)
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:100], 5)
    fr = Frame(s.ctx, prob)
    unit, U = fr.units(882)
    for step_name in ("units", "coarsened"):
        a = _built(s.ctx, unit, U) if step_name == "units" else _coarsened(s.ctx, *zl.coarse_map(fr.sizes, 882, 3))
        n = a["entries_out"]
        for step in (1, 1000, 997):
            parts = [s.ctx.assembly_contacts_fetch(o, min(step, n - o)) for o in range(0, n, step)]
            assert np.array_equal(np.concatenate([p[0] for p in parts]), a["col"]) and np.array_equal(np.concatenate([p[1] for p in parts]), a["count"])
    before = s.ctx.contact_map_order()
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:50], 5)
    assert not np.array_equal(s.ctx.contact_map_order(), before)
    col, count = s.ctx.assembly_contacts_fetch(0, a["entries_out"])
    assert np.array_equal(col, a["col"]) and np.array_equal(count, a["count"])
    s.ctx.assembly_contacts_release()
    s.free_gpu()


def test_the_timed_coarsening_leaves_the_snapshot_and_its_checksum_is_the_results():
    from instagraal_amd import hip_lib, zoom_levels as zl

    prob, s = _sampler("small", seed=19)
    fr = Frame(s.ctx, prob)
    unit, U = fr.units(BINSIZES[0])
    fine = _built(s.ctx, unit, U)
    m, C_ = zl.coarse_map(fr.sizes, BINSIZES[0], 3)
    ms, ck = s.ctx.debug_zoom_time(2, m, C_)
    assert ms.shape == (2, len(hip_lib.ZOOM_PASSES)) and (ms[:, :2] > 0).all() and (ms[:, 5] > 0).all()
    col, count = s.ctx.assembly_contacts_fetch(0, fine["entries_out"])  # the snapshot is as it was
    assert np.array_equal(col, fine["col"]) and np.array_equal(count, fine["count"])
    want = zl.coarsen_host(fine["rowptr"], fine["col"], fine["count"], m, C_)
    words = np.concatenate([want[0], want[1].astype(np.int64), want[2]]).tolist()
    total = sum(w * (k + 1) for k, w in enumerate(words)) % (1 << 64)
    assert ck == (total - (1 << 64) if total >= 1 << 63 else total)
    _, ck2 = s.ctx.debug_zoom_time(1)  # two units to one
    half = zl.coarsen_host(fine["rowptr"], fine["col"], fine["count"], np.arange(U) // 2, (U + 1) // 2)
    got = _coarsened(s.ctx, np.arange(U) // 2, (U + 1) // 2)
    assert all(got[k].tobytes() == w.tobytes() for k, w in zip(ARRAYS, half)) and ck2 != ck
    with pytest.raises(hip_lib.HipError, match="units"):
        s.ctx.debug_zoom_time(1, m, C_)  # (the snapshot is the coarsened one now)
    s.ctx.assembly_contacts_release()
    with pytest.raises(hip_lib.HipError, match="nothing to coarsen"):
        s.ctx.debug_zoom_time(1)
    s.free_gpu()


def test_a_run_with_write_zoom_levels_in_the_middle_is_the_run_without(tmp_path):
    outs = []
    for with_it in (False, True):
        prob, s = _sampler("small", seed=3)
        frags = np.random.permutation(prob.n_frags)[:200]
        res = [s.step_sampler_batch(frags[:100], 5)]
        if with_it:
            made = s.write_zoom_levels(str(tmp_path / "zoom"), resolutions=(3556, 7112, 35560), balance=dict(min_nnz=2))
            assert [m["made"] for m in made] == [("direct",), ("coarsen", 2), ("coarsen", 5), ("coarsen", "scaffolds")]
        res.append(s.step_sampler_batch(frags[100:], 5))
        sums, ints = s.ctx.debug_globals()
        outs.append((np.concatenate(res).tobytes(), s.gpu_vect_frags.copy_from_gpu().soa17(), sums.tolist(), ints.tolist(),
                     np.random.get_state()[1].copy(), np.random.get_state()[2]))
        s.free_gpu()
    a, b = outs
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3] and np.array_equal(a[4], b[4]) and a[5] == b[5]


# ---- balancing over a caller's units

MIN_NNZ = 3  # lowered from balance.DEFAULTS' 10: at scaffold level `small` has fewer scaffolds than that, everything would be masked


@pytest.mark.parametrize("what", (BINSIZES[1], "scaffold"))
def test_balance_build_units(what):
    import test_hip_balance as tb
    from instagraal_amd import balance as bal

    prob, s = _sampler("small", seed=41)
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:100], 5)
    fr = Frame(s.ctx, prob)
    unit, U = fr.units(what)
    key = np.where(fr.position >= 0, unit[np.maximum(fr.position, 0)], -1)
    for d in (1, 2):
        want = bal.entries_host(key, U, prob.coo_row, prob.coo_col, prob.coo_cnt, d)
        got = s.ctx.balance_build_units(unit, U, d)
        got["col"], got["count"] = s.ctx.balance_fetch(0, got["entries_out"])
        tb._assert_rows(got, want, (what, d))
    masked = bal.mask_units(want["nnz"], want["total"], MIN_NNZ)
    assert masked.sum() * 2 < U, (int(masked.sum()), U)  # the rule alone masks fewer than half the units
    b0 = np.where(masked, 0.0, 1.0)
    rule = bal.iterate(want["rowptr"], want["col"], want["count"], b0, 1e-5, 200)
    run = s.ctx.balance_run(b0, 1e-5, 200)
    tb._assert_run(run, rule, what)
    w_rule, _ = bal.finish(rule["b"], rule["marg_final"], masked)
    res = s._balance_units(unit, U, min_nnz=MIN_NNZ)
    assert np.array_equal(res["weight"].view(np.uint64), w_rule.view(np.uint64)) and res["n_iters"] == rule["n_iters"] > 0
    with pytest.raises(Exception, match="not monotone"):
        s.ctx.balance_build_units(unit[::-1].copy(), U, 2)
    with pytest.raises(Exception, match="nothing is built"):
        s.ctx.balance_fetch(0, 1)
    assert s.balance(level="bin")["n_units"] > 0  # the three levels behave as before
    s.free_gpu()


# ---- the sampler layer and end to end


def _read_level(folder):
    from instagraal_amd import zoom_levels as zl

    return {f: open(os.path.join(folder, f)).read() for f in sorted(os.listdir(folder))}, zl.read_pixels(os.path.join(folder, "pixels.tsv"))


def test_the_sampler_layer_against_the_writers_applied_to_the_rule(tmp_path):
    import scipy.sparse as sp

    from instagraal_amd import assembly_contacts as ac, synth, zoom_levels as zl

    prob0 = synth.make_problem(*synth.CONFIGS["tiny"])
    M = prob0.n_sub_frags
    dg = np.zeros(M, np.int32)
    dg[::5] = 1 + np.arange(M)[::5] % 9
    prob, s = _sampler("tiny", seed=18, sparse_matrix=(prob0.sub_csr + sp.diags(dg, format="csr")).tocsr())
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:100], 5)
    fr = Frame(s.ctx, prob)
    sym_d = np.asarray(s.sparse_matrix.diagonal()).astype(np.int64)[fr.order]
    resolutions = (882, 3528, 4000, 12000)
    made = s.write_zoom_levels(str(tmp_path / "dev"), resolutions=resolutions, block_rows=33)
    assert [m["made"] for m in made] == [("direct",), ("coarsen", 4), ("direct",), ("coarsen", 3), ("coarsen", "scaffolds")]
    for what, one in zip(resolutions + ("scaffold",), made):
        unit, U = fr.units(what)
        want = fr.rule(unit, U)
        diag = np.zeros(U, np.int64)
        np.add.at(diag, unit, sym_d)
        bins = zl.scaffold_table(fr.table) if what == "scaffold" else zl.binnify(fr.sizes, what)
        where = str(tmp_path / "rule" / str(what))
        n = zl.write_level(where, bins, want["rowptr"], zl.fetch_of(want["col"], want["count"]), diag=diag)
        files, px = _read_level(one["folder"])
        assert files == _read_level(where)[0] and sorted(files) == ["bins.bed", "chrom.sizes", "pixels.tsv"]
        assert one["pixels_written"] == n and one["contacts_diagonal"] == int(sym_d.sum()) and int(px[2].sum()) == want["contacts_kept"] + int(sym_d.sum())
        assert one["units_without_position"] == zl.units_without_position(unit, U) and all(one[k] == want[k] for k in CARRIED)
        got = s.scaffold_contacts() if what == "scaffold" else s.resolution_contacts(what)
        rp, cc, vv = ac.merge_diagonal(0, want["rowptr"], want["col"], want["count"], diag)
        assert got["rowptr"].tobytes() == rp.tobytes() and got["col"].tobytes() == cc.tobytes() and got["count"].tobytes() == vv.tobytes()
        assert got["bins"].tobytes() == bins.tobytes() and got["units_without_position"] == one["units_without_position"]
        assert all(got[k] == want[k] for k in ac.SCALARS) and np.array_equal(got["unit"], unit)
    assert made[0]["units_without_position"] > 0
    assert one["folder"] == os.path.join(str(tmp_path / "dev"), "scaffolds") and made[0]["folder"] == os.path.join(str(tmp_path / "dev"), "resolutions", "882")
    own = s.resolution_contacts(units=(fr.units(3528)[0], fr.units(3528)[1]), diagonal=False, balance=dict(min_nnz=2))
    lean = fr.rule(*fr.units(3528))
    assert all(own[k].tobytes() == lean[k].tobytes() for k in ARRAYS) and own["bins"] is None and own["weight"].size == lean["n_units"]
    assert np.isfinite(own["balanced"]).any()
    with pytest.raises(ValueError):
        s.resolution_contacts()
    with pytest.raises(ValueError):
        s.write_zoom_levels(str(tmp_path / "bad"), resolutions=(20, 10))
    with pytest.raises(Exception, match="nothing is built"):  # released at the end and on any error
        s.ctx.assembly_contacts_fetch(0, 1)
    s.free_gpu()


def test_run_instagraal_save_resolutions(tmp_path):
    from instagraal_amd import synth
    from instagraal_amd.simulation import run_instagraal

    data = str(tmp_path / "data")
    synth.write_text_dataset(data, n_contigs=10, mean_frags=110, seed=7, contacts_per_frag=40)
    np.random.seed(17)
    res = (3556, 7112, 35560)
    p2 = run_instagraal(data, os.path.join(data, "genome.fa"), output_folder=str(tmp_path / "out"), level=2, cycles=1, bomb=True, save_resolutions=res)
    s = p2.simulation.sampler
    root = os.path.join(p2.simulation.output_folder, "zoom_levels")
    assert sorted(os.listdir(root)) == ["resolutions", "scaffolds"] and sorted(os.listdir(os.path.join(root, "resolutions")), key=int) == [str(b) for b in res]
    from instagraal_amd import zoom_levels as zl

    assert zl.plan(res) == [("direct",), ("coarsen", 2), ("coarsen", 5)]
    for B in res:  # the files are those of three direct builds
        direct = s.write_zoom_levels(str(tmp_path / "direct" / str(B)), resolutions=(B,), scaffolds=B == res[-1])
        assert direct[0]["made"] == ("direct",)
        assert _read_level(os.path.join(root, "resolutions", str(B)))[0] == _read_level(direct[0]["folder"])[0]
    assert _read_level(os.path.join(root, "scaffolds"))[0] == _read_level(direct[1]["folder"])[0]
    px = zl.read_pixels(os.path.join(root, "scaffolds", "pixels.tsv"))
    assert px[2].sum() > 0 and np.all(px[0] <= px[1])
