"""GPU tests of the balancing's rows from a built map (ig_balance_build_snapshot, ig_debug_balance_snapshot; sampler.pairs_balance,
write_pairs_zoom_levels(balance=...), resolution_contacts / write_zoom_levels with source "snapshot" and the modes "cis" / "trans") against
the rule's host statement (balance.entries_of_rows, balance.balance_rows_host).  Every comparison is exact: the arrays' bytes."""
import ctypes as C
import filecmp
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS = ("rowptr", "nnz", "total")
LIMITS = ((0, 0), (4, 16), (64, 65), (1, 1))  # the sort forms: the defaults, then lowered as test_hip_pyramid_levels.py lowers them


def _sampler(cfg, seed=None, **extra):
    import test_hip_assembly_contacts as ta

    return ta._sampler(cfg, seed, **extra)


def _csr(U, entries):
    """(u, v, c) with u <= v, distinct -> rowptr int64 [U + 1], col int32, count int64"""
    e = sorted(entries)
    assert len({(u, v) for u, v, _ in e}) == len(e) and all(0 <= u <= v < U for u, v, _ in e)
    rowptr = np.zeros(U + 1, np.int64)
    for u, _, _ in e:
        rowptr[u + 1] += 1
    return np.cumsum(rowptr), np.array([v for _, v, _ in e], np.int32), np.array([c for _, _, c in e], np.int64)


def _by_lengths(U, lengths, seed):
    """row u holds lengths[u] entries at seeded columns of u .. U - 1, seeded counts (some beyond 32 bits)"""
    rng = np.random.default_rng(seed)
    entries = []
    for u, n in enumerate(lengths):
        for v in sorted(rng.choice(np.arange(u, U), n, replace=False).tolist()):
            entries.append((u, v, int(rng.integers(0, 50)) if rng.random() < 0.9 else int(rng.integers(1 << 33, 1 << 36))))
    return _csr(U, entries)


def _snapshot(ctx, U):
    """the handle's snapshot of U units as it lies on the device -> (rowptr, col, count)"""
    from instagraal_amd import hip_lib

    rowptr = np.zeros(U + 1, np.int64)
    hip_lib._ck(hip_lib.lib().ig_assembly_contacts_rows(ctx._h, hip_lib._p(rowptr), C.c_int64(rowptr.size)))
    return (rowptr,) + ctx.assembly_contacts_fetch(0, int(rowptr[-1]))


def _assert_rows(ctx, got, want, what):
    from instagraal_amd import balance as bal

    for k in ROWS:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (what, k)
    col, count = ctx.balance_fetch(0, got["n_entries"])
    assert col.dtype == want["col"].dtype and col.tobytes() == want["col"].tobytes() and count.tobytes() == want["count"].tobytes(), what
    assert [got[k] for k in bal.SNAPSHOT_SCALARS] == [want[k] for k in bal.SNAPSHOT_SCALARS], (what, got, want)
    assert got["n_entries"] == got["entries_out"] == got["entries"] == int(got["rowptr"][-1])


def _check(ctx, csr, what, ignore_diags=2, mode="all", group=None):
    """the debug build over the data against the rule; the data, loaded as the snapshot, is intact behind it"""
    from instagraal_amd import balance as bal

    rowptr, col, count = csr
    want = bal.entries_of_rows(rowptr, col, count, ignore_diags, group, mode)
    assert bal.snapshot_observed_total(want) == sum(count.tolist())
    got = ctx.debug_balance_snapshot(rowptr, col, count, ignore_diags, mode, group)
    _assert_rows(ctx, got, want, what)
    for a, b in zip(_snapshot(ctx, rowptr.size - 1), csr):
        assert a.tobytes() == b.tobytes(), (what, "the snapshot behind the build")
    return got


@pytest.fixture(scope="module")
def ctx():
    from instagraal_amd import hip_lib

    c = hip_lib.Context()
    yield c
    c.close()


def test_the_smallest_maps(ctx):
    got = _check(ctx, _csr(1, [(0, 0, 5)]), "U = 1, the diagonal only")
    assert got["entries"] == 0 and got["within_observed"] == 5 and got["rowptr"].tolist() == [0, 0]
    got = _check(ctx, _csr(2, [(0, 1, 7)]), "U = 2, ignore_diags 1", ignore_diags=1)
    assert got["entries"] == 2 and got["kept_observed"] == 7 and got["total"].tolist() == [7, 7]
    got = _check(ctx, _csr(2, [(0, 1, 7)]), "U = 2, ignore_diags 2", ignore_diags=2)
    assert got["entries"] == 0 and got["band_observed"] == 7
    _check(ctx, _csr(0, []), "no unit")
    _check(ctx, _csr(5, []), "no entry")


@pytest.mark.parametrize("K", (63, 64, 65, 4097))
def test_entries_around_a_wave_and_a_block(K):
    """rows of 64 entries: every row starts on lane 0 of a wave, the fifth on a workgroup's first thread; then the same entries with the
    first row one shorter, so that every later row starts on lane 63"""
    from instagraal_amd import hip_lib

    ctx = hip_lib.Context()
    U = 300
    for first in (64, 63):
        lengths, left = [], K
        while left:
            lengths.append(min(first if not lengths else 64, left))
            left -= lengths[-1]
        csr = _by_lengths(U, lengths + [0] * (U - len(lengths)), K + first)
        assert csr[1].size == K and (K < 257 or first != 64 or 256 in csr[0])
        for d in (1, 2, 9):
            _check(ctx, csr, (K, first, d), ignore_diags=d)
    ctx.close()


def test_empty_rows_and_full_rows(ctx):
    # runs of empty rows before, between and behind the entries; the first and the last row empty, then both held
    _check(ctx, _by_lengths(40, [0, 0, 0, 5, 0, 0, 0, 0, 7, 1, 0, 0, 3] + [0] * 27, 1), "empty rows at both ends", ignore_diags=1)
    _check(ctx, _by_lengths(40, [6] + [0] * 17 + [4, 0, 0, 2] + [0] * 17 + [1], 2), "the first and the last row hold entries", ignore_diags=1)
    _check(ctx, _csr(9, [(8, 8, 3)]), "the last row's diagonal alone")
    _check(ctx, _csr(9, [(0, 8, 3)]), "the corner alone")
    # a full first row: 64 and 65 upper entries (a whole wave of one row, and one more)
    for n in (64, 65):
        _check(ctx, _csr(n + 1, [(0, v, v) for v in range(1, n + 1)]), ("a full first row", n), ignore_diags=1)
        _check(ctx, _csr(n + 1, [(0, v, v) for v in range(0, n + 1)] + [(u, u + 1, 2) for u in range(1, n)]), ("a full first row and a band", n), ignore_diags=2)


@pytest.mark.parametrize("U", (70, 300))
def test_a_hub_column_in_every_sort_form(U):
    """every row holds the last unit: the last row's mirrored entries come from U - 1 source rows, one atomic each; the other rows are
    short.  The limits put the hub's row into the lds form and the long form (merges from runs of 16, 65 and 1)"""
    from instagraal_amd import hip_lib

    ctx = hip_lib.Context()
    entries = [(u, U - 1, 1 + u) for u in range(U - 1)] + [(u, u + 3, 2) for u in range(0, U - 5, 2)] + [(u, u, 9) for u in range(0, U, 7)]
    for short_max, lds_max in LIMITS:
        ctx.debug_assembly_contacts_limits(short_max, lds_max)
        for d in (1, 2):
            got = _check(ctx, _csr(U, entries), (U, short_max, lds_max, d), ignore_diags=d)
            assert got["nnz"][U - 1] == U - 1 - (d - 1)
    ctx.debug_assembly_contacts_limits(0, 0)
    ctx.close()


def test_counts_beyond_32_bits_and_totals_around_2_53(ctx):
    from instagraal_amd import balance as bal, hip_lib

    got = _check(ctx, _csr(4, [(0, 2, 1 << 40), (1, 3, 3)]), "an entry of 2^40")
    assert got["total"].tolist() == [1 << 40, 3, 1 << 40, 3] and ctx.balance_fetch(0, 4)[1].tolist() == [1 << 40, 3, 1 << 40, 3]
    top = (1 << 53) - 1
    got = _check(ctx, _csr(5, [(0, 2, top - 5), (0, 3, 5), (1, 4, 1)]), "a total of 2^53 - 1")
    assert got["total"][0] == top
    csr = _csr(5, [(0, 2, top - 5), (0, 3, 6), (1, 4, 1)])
    with pytest.raises(ValueError, match="2\\^53"):
        bal.entries_of_rows(*csr)
    with pytest.raises(hip_lib.HipError, match="2\\^53"):
        ctx.debug_balance_snapshot(*csr)
    with pytest.raises(hip_lib.HipError, match="nothing is built"):
        ctx.balance_fetch(0, 1)
    for a, b in zip(_snapshot(ctx, 5), csr):  # the refusal left the loaded snapshot as it was
        assert a.tobytes() == b.tobytes()
    _check(ctx, _csr(5, [(0, 2, top - 5), (0, 3, 6), (1, 4, 1)]), "the same inside the band", ignore_diags=4)


def test_the_three_modes(ctx):
    U = 97
    csr = _by_lengths(U, np.random.default_rng(5).integers(0, 12, U).clip(0, np.arange(U, 0, -1)).tolist(), 6)
    uneven = np.repeat(np.arange(6), (1, 40, 2, 30, 1, 23))
    for name, group in (("groups of one", np.arange(U)), ("one group", np.full(U, 3)), ("uneven groups", uneven), ("groups in any order", uneven[::-1] * 5 + 1)):
        for mode in ("all", "cis", "trans"):
            for d in (1, 3):
                got = _check(ctx, csr, (name, mode, d), ignore_diags=d, mode=mode, group=group)
                if (name, mode) in (("groups of one", "cis"), ("one group", "trans")):
                    assert got["entries"] == 0 and got["other_observed"] > 0
                if mode == "all" or (name, mode) in (("groups of one", "trans"), ("one group", "cis")):
                    assert got["other_observed"] == 0
    assert _check(ctx, csr, "mode all reads no group", mode="all", group=None)["entries"] > 0


def test_every_refusal_leaves_the_handle_usable_and_the_snapshot_as_it_was():
    from instagraal_amd import balance as bal, hip_lib
    from instagraal_amd.sampler import PARAM_NAMES

    ctx = hip_lib.Context()
    with pytest.raises(hip_lib.HipError, match="ig_balance_build_snapshot: no snapshot"):
        ctx.balance_build_snapshot()
    csr = _by_lengths(30, [3] * 20 + [0] * 10, 8)
    group = np.arange(30) // 4
    _check(ctx, csr, "before the refusals")

    def refused(call, words):
        with pytest.raises(hip_lib.HipError, match=words):
            call()
        with pytest.raises(hip_lib.HipError, match="nothing is built"):
            ctx.balance_fetch(0, 1)
        for a, b in zip(_snapshot(ctx, 30), csr):
            assert a.tobytes() == b.tobytes(), words
        assert ctx.balance_build_snapshot(1)["entries"] == ctx.debug_balance_snapshot(*csr, ignore_diags=1)["entries"] > 0  # the next builds work

    def raw(mode, g, n):
        nu, ne, sc = C.c_int64(), C.c_int64(), np.zeros(8, np.int64)
        hip_lib._ck(hip_lib.lib().ig_balance_build_snapshot(ctx._h, C.c_int32(2), C.c_int32(mode), hip_lib._p(g), C.c_int64(n), C.byref(nu), C.byref(ne), hip_lib._p(sc)))

    for d in (0, -1):
        refused(lambda: ctx.balance_build_snapshot(d), "ignore_diags")
    for m in (-1, 3):
        refused(lambda: raw(m, None, 0), "mode is 0 \\(all\\), 1 \\(cis\\) or 2 \\(trans\\)")
    refused(lambda: ctx.balance_build_snapshot(2, "cis"), "needs the group")
    refused(lambda: ctx.balance_build_snapshot(2, "trans", group[:-1]), "groups are for 29 units, the snapshot has 30")
    bad = group.copy()
    bad[7] = -1
    refused(lambda: ctx.balance_build_snapshot(2, "cis", bad), "negative group")
    # the debug entry checks its data on the host
    for data, words in (((csr[0], csr[1][::-1].copy(), csr[2]), "column|ascend"), ((csr[0][::-1].copy(), csr[1], csr[2]), "rowptr"),
                        ((csr[0], csr[1], -csr[2] - 1), "negative count")):
        with pytest.raises(hip_lib.HipError, match=words):
            ctx.debug_balance_snapshot(*data)
    # a handle that holds a shard: its snapshot would be that shard's
    _check(ctx, csr, "a snapshot in front of the shard")
    ctx.set_shard(1, 2)
    with pytest.raises(hip_lib.HipError, match="ig_balance_build_snapshot.*shard 1 of 2"):
        ctx.balance_build_snapshot(2)
    for a, b in zip(_snapshot(ctx, 30), csr):
        assert a.tobytes() == b.tobytes()
    with pytest.raises(hip_lib.HipError, match="ig_debug_balance_snapshot.*shard 1 of 2"):
        ctx.debug_balance_snapshot(*csr)
    ctx.set_shard(0, 1)
    _check(ctx, csr, "behind the shard")
    # counts of 2^53 and more are refused one by one by the debug entry (four of 2^62 in a row would wrap its 64-bit total to 0)
    wrap = _csr(6, [(0, v, 1 << 62) for v in (2, 3, 4, 5)])
    with pytest.raises(ValueError, match="2\\^53"):
        bal.entries_of_rows(*wrap)
    with pytest.raises(hip_lib.HipError, match="counts 2\\^53 or more"):
        ctx.debug_balance_snapshot(*wrap)
    lower = (np.array([0, 0, 1], np.int64), np.array([0], np.int32), np.array([4], np.int64))
    with pytest.raises(hip_lib.HipError, match="upper-triangular"):
        ctx.debug_balance_snapshot(*lower)
    with pytest.raises(hip_lib.HipError, match="mode is one of"):
        ctx.debug_balance_snapshot(*csr, mode="both")
    ctx.close()
    # a level 0 snapshot (packed words), and a nuisance step in flight
    prob, s = _sampler("tiny", seed=41)
    s.ctx.assembly_contacts("sub")
    with pytest.raises(hip_lib.HipError, match="level 0 snapshot cannot be balanced"):
        s.ctx.balance_build_snapshot()
    s.ctx.assembly_contacts("bin")
    cands = s.return_neighbours(3, 5)
    p8 = np.array([float(s.param_simu[k][0]) for k in PARAM_NAMES], np.float32)
    s.ctx.nuis_begin(3, sorted(int(x) for x in cands if x != 3), p8, s.mean_kb())
    with pytest.raises(hip_lib.HipError, match="ig_balance_build_snapshot.*in flight"):
        s.ctx.balance_build_snapshot()
    s.ctx.nuis_end()
    res = s.ctx.assembly_contacts("bin")  # (the step's move may have changed the genome)
    before = s.ctx.assembly_contacts_fetch(0, res["n_entries"])
    built = s.ctx.balance_build_snapshot()
    _assert_rows(s.ctx, built, bal.entries_of_rows(res["rowptr"], *before), "the level 1 snapshot of a genome")  # byte for byte
    after = s.ctx.assembly_contacts_fetch(0, res["n_entries"])
    assert built["entries"] > 0 and built["entries_in"] == res["n_entries"] and before[0].size and all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
    ms = s.ctx.debug_balance_snapshot_time(2)
    assert ms.shape == (2, len(hip_lib.BALANCE_SNAPSHOT_PASSES)) and (ms[:, 0] > 0).all() and (ms[:, -1] > 0).all()
    s.ctx.balance_release()
    s.ctx.assembly_contacts_release()
    s.free_gpu()


# ---------------------------------------------------------------- through the sampler, on `tiny`

KW = dict(min_nnz=2, tol=1e-6, max_iters=300)


def _assert_balanced(got, want, what):
    for k in ("weight", "variance", "masked"):
        assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), (what, k)
    assert got["n_iters"] == want["n_iters"] and got["converged"] == want["converged"] and (got["scale"] == want["scale"] or (got["scale"] != got["scale"] and want["scale"] != want["scale"])), what  # (equal, or both nan)
    for k in ("within_observed", "band_observed", "other_observed", "kept_observed", "entries"):
        assert got[k] == want[k], (what, k)


def _tree(folder):
    return sorted(os.path.relpath(os.path.join(d, f), folder) for d, _, fs in os.walk(folder) for f in fs)


def _assert_pairs_session(s, prob, what, tmp_path, seed):
    import test_hip_pairs_lift as tp
    from instagraal_amd import assembly_contacts as ac, balance as bal, pairs_lift as pl, zoom_levels as zl

    table = s.pairs_begin()
    c1, p1, c2, p2, strands = tp._pairs(table, 4097, seed)
    lifted = pl.lift_host(table, c1, p1, c2, p2)
    s.lift_pairs(c1, p1, c2, p2, strands)
    sizes = ac.chrom_sizes(table["table_sub"])
    B = tp.BINSIZES[0]
    # pairs_balance at a bin size, at "bin" and at "sub"; the modes
    for units in (B, "bin", "sub"):
        px = pl.pixels_host(lifted, table, units)
        bins = s._pairs_bins(*pl.check_units(table, units)[:2])
        for mode in ("all", "cis", "trans"):
            kw = dict(binsize=units) if units == B else dict(units=units)
            got = s.pairs_balance(None, mode=mode, **kw, **KW)
            want = bal.balance_rows_host(px["rowptr"], px["col"], px["count"], bins["contig"], mode, **KW)
            for k in ("rowptr", "col", "count"):
                assert got[k].tobytes() == px[k].tobytes(), (what, units, k)
            _assert_balanced(got, want, (what, units, mode))
            assert got["balance_scalars"] == {k: want[k] for k in bal.SNAPSHOT_SCALARS}
            assert got["balanced"].tobytes() == bal.balanced(px["count"], ac.rows_of(px["rowptr"]), px["col"], want["weight"]).tobytes()
            assert mode != "all" or want["n_iters"] > 1
    with pytest.raises(ValueError, match="cis"):
        s.pairs_balance(None, units="scaffold", mode="cis")
    with pytest.raises(NotImplementedError, match="balanc"):
        s.pairs_contacts(None, binsize=B, balance=True)
    # the snapshot is the same bytes before and behind a balancing, and so is a coarsening behind it
    res = s.ctx.pairs_pixels("binsize", B)
    before = s.ctx.assembly_contacts_fetch(0, res["n_entries"])
    s._balance_snapshot(**KW)
    after = s.ctx.assembly_contacts_fetch(0, res["n_entries"])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
    co = s.ctx.assembly_contacts_coarsen(*zl.coarse_map(sizes, B, 7))
    co["col"], co["count"] = s.ctx.assembly_contacts_fetch(0, co["n_entries"])
    want = pl.pixels_host(lifted, table, 7 * B)
    assert all(co[k].tobytes() == want[k].tobytes() for k in ("rowptr", "col", "count"))
    s.ctx.assembly_contacts_release()
    # the zoom levels: weights.tsv of every level -- built, coarsened, the scaffolds -- is the rule's; the other files do not change
    levels = (B, 7 * B, 11 * B)  # direct, coarsened, direct
    plain, balanced = str(tmp_path / (what + "_plain")), str(tmp_path / (what + "_balanced"))
    s.write_pairs_zoom_levels(plain, None, levels)
    for mode in ("all", "cis"):
        folder = balanced + "_" + mode
        out = s.write_pairs_zoom_levels(folder, None, levels, balance=dict(KW, mode=mode))
        assert [o["made"][0] for o in out] == ["direct", "coarsen", "direct", "coarsen"]
        extra = []
        for o in out:
            units = "scaffold" if o["level"] == "scaffolds" else o["level"]
            px = pl.pixels_host(lifted, table, units)
            bins = zl.scaffold_table(table["table_sub"]) if units == "scaffold" else zl.binnify(sizes, units)
            path = os.path.join(o["folder"], "weights.tsv")
            if units == "scaffold" and mode == "cis":
                assert o["balanced"] is False and not os.path.exists(path)
                continue
            extra.append(os.path.relpath(path, folder))
            want = str(tmp_path / "want.tsv")
            bal.write_snapshot_weights(want, bins, bal.balance_rows_host(px["rowptr"], px["col"], px["count"], bins["contig"], mode, **KW))
            assert o["balanced"] is True and open(path, "rb").read() == open(want, "rb").read(), (what, mode, units)
            last = open(path).read().splitlines()[-1]
            assert last.startswith("# source=snapshot mode=%s other_observed=" % mode) and (mode == "all") == (" other_observed=0 " in last)
            assert bal.read_weights(path)[0].size == bins.size
        assert sorted(set(_tree(folder)) - set(_tree(plain))) == sorted(extra) and set(_tree(plain)) <= set(_tree(folder))
        for f in _tree(plain):
            assert filecmp.cmp(os.path.join(plain, f), os.path.join(folder, f), shallow=False), (what, mode, f)
    s.pairs_end()


def test_pairs_balance_and_the_zoom_levels_on_tiny_fresh_and_behind_moves_with_flips(tmp_path):
    prob, s = _sampler("tiny", seed=12)
    _assert_pairs_session(s, prob, "fresh", tmp_path, 1)
    s.bomb_the_genome()
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:150], 5)
    g = s.gpu_vect_frags.copy_from_gpu()
    assert (g.ori == -1).sum() >= 3 and np.unique(g.id_c).size > 20
    _assert_pairs_session(s, prob, "moved", tmp_path, 2)
    s.free_gpu()


def test_the_contacts_maps_by_both_sources(tmp_path):
    import test_hip_zoom_levels as tz
    from instagraal_amd import balance as bal

    prob, s = _sampler("tiny", seed=14)
    s.bomb_the_genome()
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:100], 5)
    B = 3556
    a = s.resolution_contacts(B, balance=dict(KW))
    b = s.resolution_contacts(B, balance=dict(KW, source="snapshot"))
    assert np.isfinite(a["weight"]).sum() > 3 and a["weight"].tobytes() == b["weight"].tobytes() and a["balanced"].tobytes() == b["balanced"].tobytes()
    for k in ("rowptr", "col", "count"):
        assert a[k].tobytes() == b[k].tobytes()
    a, b = s.resolution_contacts(B, balance=True), s.resolution_contacts(B, balance={"source": "snapshot"})  # the defaults, as the issue writes them
    assert a["weight"].tobytes() == b["weight"].tobytes() and a["balanced"].tobytes() == b["balanced"].tobytes()
    # the modes against the rule over the map without its diagonal (the device holds the strict upper triangle)
    fr = tz.Frame(s.ctx, prob)
    unit, U = fr.units(B)
    px = fr.rule(unit, U)
    for mode in ("cis", "trans"):
        got = s.resolution_contacts(B, balance=dict(KW, mode=mode))
        want = bal.balance_rows_host(px["rowptr"], px["col"], px["count"], a["bins"]["contig"], mode, **KW)
        assert got["weight"].tobytes() == want["weight"].tobytes(), mode
    with pytest.raises(ValueError, match="cis"):
        s.resolution_contacts(units="scaffold", balance=dict(mode="cis"))
    with pytest.raises(ValueError, match="source"):
        s.resolution_contacts(B, balance=dict(mode="cis", source="contacts"))
    # write_zoom_levels: the same files by both sources, weights.tsv included
    one, two = str(tmp_path / "contacts"), str(tmp_path / "snapshot")
    s.write_zoom_levels(one, (B, 2 * B), balance=dict(KW))
    s.write_zoom_levels(two, (B, 2 * B), balance=dict(KW, source="snapshot"))
    files = _tree(one)
    assert files == _tree(two) and sum(f.endswith("weights.tsv") for f in files) == 3
    for f in files:
        if f.endswith("weights.tsv"):  # every unit's line is the same bytes; the last line names each route's own scalars
            a, b = (open(os.path.join(d, f)).read().splitlines() for d in (one, two))
            assert a[:-1] == b[:-2] and len(a) > 3 and a[-1].startswith("# level=units") and b[-2].startswith("# level=units"), f
            assert " unplaced_observed=" in a[-1] and " unplaced_observed=" not in b[-2] and a[-1].split(" unplaced_observed=")[0] == b[-2].split(" within_observed=")[0]
            assert b[-1].startswith("# source=snapshot mode=all other_observed=0 entries_in=")
        else:
            assert filecmp.cmp(os.path.join(one, f), os.path.join(two, f), shallow=False), f
    out = s.write_zoom_levels(str(tmp_path / "cis"), (B,), balance=dict(KW, mode="cis"))
    assert [o["balanced"] for o in out] == [True, False] and not os.path.exists(os.path.join(out[1]["folder"], "weights.tsv"))
    s.free_gpu()


def test_a_run_with_pairs_and_balance_pairs(tmp_path):
    import test_hip_pairs_lift as tp
    from instagraal_amd import synth
    from instagraal_amd.simulation import run_balanced_pairs, run_instagraal

    data = str(tmp_path / "data")
    synth.write_text_dataset(data, n_contigs=10, mean_frags=110, seed=7, contacts_per_frag=40)
    names, lengths = tp._contigs_of(data)
    rng = np.random.default_rng(3)
    n = 3000
    k1 = rng.integers(0, len(names), n)
    k2 = np.where(rng.random(n) < 0.7, k1, rng.integers(0, len(names), n))
    src = str(tmp_path / "in.pairs")
    with open(src, "w") as f:
        f.write("## pairs format v1.0\n#columns: readID chr1 pos1 chr2 pos2 strand1 strand2\n")
        for i in range(n):
            f.write("r%d\t%s\t%d\t%s\t%d\t+\t-\n" % (i, names[k1[i]], rng.integers(1, lengths[k1[i]] + 1), names[k2[i]], rng.integers(1, lengths[k2[i]] + 1)))
    res = (2000, 10_000)
    kw = dict(level=2, cycles=1, bomb=True, save_resolutions=res)
    outs = {}
    for name, run in (("parent", lambda d, o: run_instagraal(d, os.path.join(d, "genome.fa"), output_folder=o, pairs=src, **kw)),
                      ("off", lambda d, o: run_balanced_pairs(d, os.path.join(d, "genome.fa"), src, output_folder=o, balance_pairs=False, **kw)),
                      ("on", lambda d, o: run_balanced_pairs(d, os.path.join(d, "genome.fa"), src, output_folder=o, balance_pairs=dict(min_nnz=2), **kw))):
        d = str(tmp_path / ("run_" + name) / "data")  # a folder of its own per run (the first run of a folder builds its pyramid there), the same name: the outputs carry it
        os.makedirs(os.path.dirname(d))
        synth.write_text_dataset(d, n_contigs=10, mean_frags=110, seed=7, contacts_per_frag=40)
        np.random.seed(17)
        p2 = run(d, str(tmp_path / name))
        outs[name] = p2.simulation.output_folder
        if name != "on":
            p2.simulation.release()
    s = p2.simulation.sampler
    # without the flag the run's folder is run_instagraal's: the same lists, the same bytes
    assert _tree(outs["off"]) == _tree(outs["parent"]) and not [f for f in _tree(outs["off"]) if f.endswith("weights.tsv")]
    for f in _tree(outs["parent"]):
        assert filecmp.cmp(os.path.join(outs["parent"], f), os.path.join(outs["off"], f), shallow=False), f
    # with it: weights.tsv per level of pairs_zoom_levels/, nothing else added, nothing else changed
    added = [os.path.join("pairs_zoom_levels", "resolutions", str(b), "weights.tsv") for b in res] + [os.path.join("pairs_zoom_levels", "scaffolds", "weights.tsv")]
    assert sorted(set(_tree(outs["on"])) - set(_tree(outs["parent"]))) == sorted(added) and set(_tree(outs["parent"])) <= set(_tree(outs["on"]))
    for f in _tree(outs["parent"]):
        assert filecmp.cmp(os.path.join(outs["parent"], f), os.path.join(outs["on"], f), shallow=False), f
    # and the weights are what the sampler writes for the final genome
    root, again = os.path.join(outs["on"], "pairs_zoom_levels"), str(tmp_path / "again")
    s.write_pairs_zoom_levels(again, src, res, balance=dict(min_nnz=2))
    assert _tree(root) == _tree(again)
    for f in _tree(root):
        assert filecmp.cmp(os.path.join(again, f), os.path.join(root, f), shallow=False), f
    s.free_gpu()
