"""GPU tests of the pyramid's contact levels (ig_pyr_begin / _matrix / _degrees / _remap / _rows / _fetch / _end, pyramid_device,
simulation.run_device_pyramid) against the rule's host statement (instagraal_amd.pyramid_levels), the host path (instagraal_amd.pyramid)
and the golden of the reference's own builder (tests/golden/pyramid_small.npz).  Every comparison is exact."""
import filecmp
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu


def _scan_chunk():
    src = open(os.path.join(ROOT, "instagraal_amd", "csrc", "ig_kernels_rows.cuh")).read()
    return int(re.search(r"#define SCAN_THREADS (\d+)", src).group(1)) * int(re.search(r"#define SCAN_ITEMS (\d+)", src).group(1))


@pytest.fixture(scope="module")
def ctx():
    from instagraal_amd import hip_lib

    c = hip_lib.Context(0)
    yield c
    c.close()


def same_tree(x, y):
    names = []
    for base, _, files in os.walk(x):
        for f in files:
            if f.startswith("pyramid.") and f.split(".")[-1] in ("npz", "hdf5"):
                continue
            rel = os.path.relpath(os.path.join(base, f), x)
            names.append(rel)
            assert os.path.exists(os.path.join(y, rel)), rel
            assert filecmp.cmp(os.path.join(base, f), os.path.join(y, rel), shallow=False), rel
    return names


def assert_level(ctx, M, n_frags, what):
    """the current level of the session is M: the three rows, their type, the rows' starts"""
    from instagraal_amd import pyramid_levels as rule

    data3, rowptr = ctx.pyr_level(piece=1000)
    want = rule.data3(M)
    assert data3.dtype == np.int32 and data3.shape == want.shape, (what, data3.shape, want.shape)
    assert np.array_equal(data3, want), what
    assert rowptr.size == n_frags + 1 and np.array_equal(rowptr, np.concatenate(([0], np.cumsum(np.bincount(M[0], minlength=n_frags))))), what


def shuffled_list(seed, n_frags, n):
    """not canonical: a > b, both (a, b) and (b, a), repeats, the diagonal, zero counts"""
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, n_frags, n), rng.integers(0, n_frags, n)
    k = n // 5
    a[:k], b[:k] = b[k:2 * k].copy(), a[k:2 * k].copy()
    a[2 * k:2 * k + k // 2] = b[2 * k:2 * k + k // 2]
    a[-k:], b[-k:] = a[:k], b[:k]
    count = rng.integers(1, 50, n)
    count[rng.integers(0, n, n // 6)] = 0
    p = rng.permutation(n)
    return a[p].astype(np.int64), b[p].astype(np.int64), count[p].astype(np.int64)


def bin_lut(n, factor=3):
    return np.arange(n) // factor, (n + factor - 1) // factor


# ---- (a) the golden's dataset, and (h) thresh_factor 0 / 1 / 3


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from instagraal_amd import synth

    g = np.load(os.path.join(GOLDEN, "pyramid_small.npz"))
    work = tmp_path_factory.mktemp("pyrdev")
    data = str(work / "data")
    nc, mf, seed, cpf = [int(x) for x in g["dataset"]]
    synth.write_text_dataset(data, n_contigs=nc, mean_frags=mf, seed=seed, contacts_per_frag=cpf)
    return g, data, work


@pytest.mark.parametrize("thresh_factor", [1, 0, 3])
def test_the_device_path_writes_the_host_paths_folders_and_the_goldens(ctx, dataset, thresh_factor):
    from instagraal_amd import pyramid, pyramid_device

    g, data, work = dataset
    host, dev = str(work / ("host%d" % thresh_factor)), str(work / ("dev%d" % thresh_factor))
    os.makedirs(host), os.makedirs(dev)
    p_host = pyramid.build_and_filter(data, 9, 3, thresh_factor=thresh_factor, output_folder=host)
    chain = pyramid_device.Chain(ctx)
    p_dev = pyramid_device.build_and_filter(data, 9, 3, thresh_factor=thresh_factor, output_folder=dev, device=ctx, _chain=chain)
    assert chain.seconds["device"] > 0.0 and chain.engine.live  # the levels came from a session of THIS context
    chain.close()
    a = same_tree(os.path.join(host, "pyramids"), os.path.join(dev, "pyramids"))
    b = same_tree(os.path.join(dev, "pyramids"), os.path.join(host, "pyramids"))
    assert sorted(a) == sorted(b) and len(a) == 9 * 4 - 1 + 3
    for lv in range(9):
        (d, n), (dh, nh) = p_dev.store.get(lv), p_host.store.get(lv)
        assert n == nh and d.dtype == np.int32 and np.array_equal(d, dh), lv
    s_dev, s_host = pyramid.SparseStore(os.path.join(dev, "pyramids", "pyramid_1_no_thresh")), pyramid.SparseStore(os.path.join(host, "pyramids", "pyramid_1_no_thresh"))
    assert np.array_equal(s_dev.get(0)[0], s_host.get(0)[0]) and s_dev.get(0)[1] == s_host.get(0)[1]
    if thresh_factor == 1:  # the golden was made with it
        for rel in g["txt_names"]:
            assert open(os.path.join(dev, "pyramids", str(rel)), "rb").read() == g["txt/" + str(rel)].tobytes(), rel
        for lv in range(9):
            assert np.array_equal(p_dev.store.get(lv)[0], g["h5/%d/data" % lv]) and p_dev.store.get(lv)[1] == int(g["h5/%d/nfrags" % lv][0, 0])
        assert (s_host.get(0)[1], p_host.store.get(0)[1]) == (1095, 1036)
    p_host.close(), p_dev.close()


def test_contigs_that_stay_unbinned(ctx, tmp_path):
    """(h) min_bin_per_contig large enough that some contigs keep their fragments: build() through the device and the host"""
    from instagraal_amd import pyramid, pyramid_device, synth

    data = str(tmp_path / "data")
    synth.write_text_dataset(data, n_contigs=6, mean_frags=60, seed=5, contacts_per_frag=8)
    n_in = [int(ln.split("\t")[2]) for ln in open(os.path.join(data, "info_contigs.txt")).read().splitlines()[1:]]
    mbc = int(np.median(n_in)) // 3
    assert any(n / 3.0 >= mbc for n in n_in) and any(n / 3.0 < mbc for n in n_in)
    host, dev = str(tmp_path / "host"), str(tmp_path / "dev")
    os.makedirs(host), os.makedirs(dev)
    pyramid.build(data, 4, 3, mbc, output_folder=host)
    pyramid_device.build(data, 4, 3, mbc, output_folder=dev, device=ctx)
    assert len(same_tree(os.path.join(host, "pyramids"), os.path.join(dev, "pyramids"))) == 4 * 4 - 1
    f = "pyramid_4_no_thresh"
    s_host, s_dev = pyramid.SparseStore(os.path.join(host, "pyramids", f)), pyramid.SparseStore(os.path.join(dev, "pyramids", f))
    for lv in range(4):
        assert np.array_equal(s_host.get(lv)[0], s_dev.get(lv)[0]) and s_host.get(lv)[1] == s_dev.get(lv)[1], lv


# ---- (b) the three sort forms and a hub column


def test_a_hub_fragment_reaches_the_short_lds_and_long_sorts(ctx):
    from instagraal_amd import pyramid_levels as rule

    n_frags, hub = 3000, 1500
    rng = np.random.default_rng(21)
    others = np.delete(np.arange(n_frags), hub)
    a = np.concatenate((np.full(others.size, hub), rng.integers(0, n_frags, 6000), np.zeros(40, np.int64), np.full(300, 7)))
    b = np.concatenate((others, rng.integers(0, n_frags, 6000), rng.integers(0, n_frags, 40), rng.integers(8, n_frags, 300)))
    count = rng.integers(0, 9, a.size)
    p = rng.permutation(a.size)
    a, b, count = a[p], b[p], count[p]
    per_row = np.bincount(np.minimum(a, b), minlength=n_frags)
    short_max, lds_max = 8, 64
    assert (per_row[per_row > 1] <= short_max).any() and ((per_row > short_max) & (per_row <= lds_max)).any() and (per_row > lds_max).sum() >= 2
    M = rule.level_matrix(a, b, count)
    want_deg = rule.degrees(M, n_frags)
    assert want_deg[hub] >= 2000  # the hub column takes a degree atomic from nearly every row in front of it
    lut, n_new = bin_lut(n_frags)
    lut = lut.copy()
    lut[100:130] = -1
    keep_ids = np.unique(lut[lut >= 0])
    lut[lut >= 0] = np.searchsorted(keep_ids, lut[lut >= 0])
    n_new = keep_ids.size
    try:
        for limits in ((short_max, lds_max), (0, 0)):
            ctx.debug_assembly_contacts_limits(*limits)
            assert ctx.pyr_begin(n_frags, a, b, count) is False
            try:
                assert ctx.pyr_matrix() == M[0].size
                assert_level(ctx, M, n_frags, limits)
                assert np.array_equal(ctx.pyr_degrees(), want_deg)
                sc_want = {}
                M1 = rule.remap(*M, lut, True, scalars=sc_want)
                assert ctx.pyr_remap(lut, n_new, True) == sc_want
                assert_level(ctx, M1, n_new, limits)
                assert np.array_equal(ctx.pyr_degrees(), rule.degrees(M1, n_new))
            finally:
                ctx.pyr_end()
    finally:
        ctx.debug_assembly_contacts_limits(0, 0)


# ---- (c) the scan's chunk boundary


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_fragments_around_a_scan_chunk(ctx, delta):
    from instagraal_amd import pyramid_levels as rule

    n_frags = _scan_chunk() + delta
    assert n_frags in (2047, 2048, 2049)
    rng = np.random.default_rng(30 + delta)
    a = np.concatenate(([0, 0, n_frags - 1], rng.integers(0, n_frags, 5000)))
    b = np.concatenate(([0, n_frags - 1, n_frags - 1], rng.integers(0, n_frags, 5000)))
    count = rng.integers(1, 100, a.size)
    M = rule.level_matrix(a, b, count)
    assert M[0][0] == 0 and M[0][-1] == n_frags - 1
    ctx.pyr_begin(n_frags, a, b, count)
    try:
        ctx.pyr_matrix()
        assert_level(ctx, M, n_frags, "level")
        assert np.array_equal(ctx.pyr_degrees(), rule.degrees(M, n_frags))
        ident = np.arange(n_frags)  # a table that keeps every fragment: the next level has as many rows, and loses entry (0, 0)
        M1 = rule.remap(*M, ident, True)
        assert ctx.pyr_remap(ident, n_frags, True)["pixels"] == M1[0].size == M[0].size - 1
        assert_level(ctx, M1, n_frags, "identity")
    finally:
        ctx.pyr_end()


# ---- (d) a list that is not canonical, (g) uploaded in pieces smaller than the list


@pytest.mark.parametrize("piece", [0, 777])
def test_a_shuffled_list_with_repeats_and_zeros(ctx, piece):
    from instagraal_amd import pyramid_levels as rule

    n_frags = 500
    a, b, count = shuffled_list(41, n_frags, 9000)
    a[0], b[0], count[0] = n_frags - 1, 3, 40000  # the first entry in file order is among the last in sorted order
    assert piece < a.size and not rule.canonical(a, b)
    lut, n_new = bin_lut(n_frags)
    ctx.debug_pyr_piece(piece)
    try:
        # the flag, the level, the degrees
        assert ctx.pyr_begin(n_frags, a, b, count) is False
        M = rule.level_matrix(a, b, count)
        assert (M[2] == 0).any() and ctx.pyr_matrix() == M[0].size
        assert_level(ctx, M, n_frags, "level")
        assert np.array_equal(ctx.pyr_degrees(), rule.degrees(M, n_frags))
        ctx.pyr_end()
        # a remap of the uploaded list itself: skip_first drops the first entry in FILE order
        ctx.pyr_begin(n_frags, a, b, count)
        sc_want = {}
        M1 = rule.remap(a, b, count, lut, True, scalars=sc_want)
        assert ctx.pyr_remap(lut, n_new, True) == sc_want and sc_want["skipped"] == 1
        assert_level(ctx, M1, n_new, "remap of the list")
        assert int(rule.remap(a, b, count, lut, False)[2].sum()) - int(M1[2].sum()) == 40000
        ctx.pyr_end()
        # its level is canonical: the device says so, and the level of the level is the level
        assert ctx.pyr_begin(n_frags, *M) is True
        assert ctx.pyr_matrix() == M[0].size
        assert_level(ctx, M, n_frags, "level of the level")
    finally:
        ctx.debug_pyr_piece(0)
        ctx.pyr_end()


# ---- (e) destroyed contigs, an empty level, one fragment


def test_destroyed_contigs_an_empty_level_and_a_single_fragment(ctx):
    from instagraal_amd import pyramid_levels as rule

    n_frags = 900
    a, b, count = shuffled_list(52, n_frags, 7000)
    lut = np.full(n_frags, -1, np.int64)
    kept = np.concatenate((np.arange(0, 200), np.arange(420, 700)))  # two "contigs" destroyed whole: 200 .. 419 and 700 .. 899
    lut[kept] = np.arange(kept.size) // 2
    n_new = kept.size // 2
    ctx.pyr_begin(n_frags, a, b, count)
    try:
        ctx.pyr_matrix()
        M = rule.level_matrix(a, b, count)
        sc_want = {}
        M1 = rule.remap(*M, lut, False, scalars=sc_want)
        assert ctx.pyr_remap(lut, n_new, False) == sc_want and sc_want["dropped_by_lut"] > 1000 and sc_want["skipped"] == 0
        assert_level(ctx, M1, n_new, "contigs destroyed")
        # everything destroyed: an empty level of no fragment, its degrees, and a further remap of it
        sc = ctx.pyr_remap(np.full(n_new, -1), 0, True)
        assert sc == dict(entries_in=M1[0].size, skipped=1, dropped_by_lut=M1[0].size - 1, entries_kept=0, pixels=0, largest_sum=0)
        data3, rowptr = ctx.pyr_level()
        assert data3.shape == (3, 0) and rowptr.tolist() == [0] and ctx.pyr_degrees().size == 0
        sc = ctx.pyr_remap(np.zeros(0, np.int32), 0, True)
        assert sc == dict(entries_in=0, skipped=0, dropped_by_lut=0, entries_kept=0, pixels=0, largest_sum=0)
        assert ctx.pyr_level()[0].shape == (3, 0)
    finally:
        ctx.pyr_end()
    # fragments that survive but have lost every contact: an empty level WITH rows
    ctx.pyr_begin(5, np.array([0, 1]), np.array([1, 0]), np.array([2, 3]))
    try:
        lut5 = np.array([-1, 0, 0, 1, 1])
        assert ctx.pyr_remap(lut5, 2, False)["pixels"] == 0
        data3, rowptr = ctx.pyr_level()
        assert data3.shape == (3, 0) and rowptr.tolist() == [0, 0, 0] and ctx.pyr_degrees().tolist() == [0, 0]
    finally:
        ctx.pyr_end()
    # a level of one fragment
    ctx.pyr_begin(1, np.zeros(4, np.int64), np.zeros(4, np.int64), np.array([1, 0, 5, 6]))
    try:
        assert ctx.pyr_matrix() == 1
        assert ctx.pyr_level()[0].tolist() == [[0], [0], [12]] and ctx.pyr_degrees().tolist() == [1]
        assert ctx.pyr_remap(np.zeros(1, np.int64), 1, False)["largest_sum"] == 12
        assert ctx.pyr_level()[0].tolist() == [[0], [0], [12]]
        assert ctx.pyr_remap(np.zeros(1, np.int64), 1, True)["pixels"] == 0
    finally:
        ctx.pyr_end()


# ---- (f) the limit of a sum, and the other refusals


def test_a_sum_of_2_to_the_31_is_refused_and_the_session_stays_usable(ctx):
    from instagraal_amd import hip_lib, pyramid_levels as rule

    top = (1 << 31) - 1
    a, b = np.array([3, 5, 5, 3, 0]), np.array([5, 3, 5, 5, 1])
    ok, over = np.array([top - 10, 4, 7, 6, 1]), np.array([top - 10, 5, 7, 6, 1])
    ctx.pyr_begin(6, a, b, ok)
    try:
        assert ctx.pyr_matrix() == 3
        assert_level(ctx, rule.level_matrix(a, b, ok), 6, "2^31 - 1")
        merge = np.array([0, 0, 1, 1, 2, 2])  # (3, 5) and (5, 5) do not meet: top and 7 stay apart
        assert ctx.pyr_remap(merge, 3, False)["largest_sum"] == top
    finally:
        ctx.pyr_end()
    ctx.pyr_begin(6, a, b, over)
    try:
        with pytest.raises(hip_lib.HipError, match=r"the sum of the pixel \(3, 5\) is 2147483648: 2\^31 or more"):
            ctx.pyr_matrix()
        with pytest.raises(rule.LevelOverflow, match=r"\(3, 5\)"):
            rule.level_matrix(a, b, over)
        # the session is still usable: the list is still the current level, and a table that drops fragment 3 gives a level
        lut = np.array([0, 1, 2, -1, 3, 4])
        M1 = rule.remap(a, b, over, lut, False)
        assert ctx.pyr_remap(lut, 5, False)["pixels"] == M1[0].size == 2
        assert_level(ctx, M1, 5, "behind a refusal")
        # a remap whose sums meet at 2^31 is refused too and leaves the current level
        ctx.pyr_end()
        ctx.pyr_begin(6, a, b, ok)
        ctx.pyr_matrix()
        with pytest.raises(hip_lib.HipError, match=r"the sum of the pixel \(0, 0\) is 2147483654"):
            ctx.pyr_remap(np.zeros(6, np.int64), 1, True)  # (the first entry, (0, 1) with count 1, is skipped)
        assert_level(ctx, rule.level_matrix(a, b, ok), 6, "behind a refused remap")
    finally:
        ctx.pyr_end()


def test_refusals_name_the_entry_and_leave_the_handle_right(ctx):
    from instagraal_amd import hip_lib

    a, b, c = np.array([0, 1, 2]), np.array([1, 2, 3]), np.array([1, 1, 1])
    for call, msg in ((lambda: ctx.pyr_matrix(), "no session"), (lambda: ctx.pyr_degrees(), "no session"), (lambda: ctx.pyr_level(), "no session"),
                      (lambda: ctx.pyr_end(), "no session"), (lambda: ctx.pyr_remap(np.zeros(4, np.int64), 1, False), "no session"),
                      (lambda: ctx.pyr_begin(3, a, b, c), r"entry 2 is \(2, 3\): ids are 0 .. 2"), (lambda: ctx.pyr_begin(4, a, -b, c), r"entry 0 is \(0, -1\)"),
                      (lambda: ctx.pyr_begin(4, a, b, np.array([1, -5, 1])), "entry 1 has the count -5"),
                      (lambda: ctx.pyr_begin(4, a, b, np.array([1, 1, 1 << 31])), "entry 2 has the count 2147483648"), (lambda: ctx.pyr_begin(0, a[:0], b[:0], c[:0]), "bad sizes")):
        with pytest.raises(hip_lib.HipError, match=msg):
            call()
    ctx.pyr_begin(4, a, b, c)
    try:
        for call, msg in ((lambda: ctx.pyr_begin(4, a, b, c), "a session is open"), (lambda: ctx.pyr_degrees(), "ig_pyr_matrix first"), (lambda: ctx.pyr_level(), "ig_pyr_matrix first"),
                          (lambda: ctx.pyr_remap(np.zeros(3, np.int64), 1, False), "the table has 3 entries, the current level 4 fragments"),
                          (lambda: ctx.pyr_remap(np.array([0, 1, 0, 1]), 2, False), "maps fragment 2 to 0"), (lambda: ctx.pyr_remap(np.array([0, 1, 2, 2]), 2, False), "maps fragment 2 to 2"),
                          (lambda: ctx.pyr_remap(np.array([0, -2, 1, 1]), 2, False), "maps fragment 1 to -2")):
            with pytest.raises(hip_lib.HipError, match=msg):
                call()
        assert ctx.pyr_matrix() == 3 and ctx.pyr_level()[0].tolist() == [[0, 1, 2], [1, 2, 3], [1, 1, 1]]
    finally:
        ctx.pyr_end()


# ---- (i) the run


def test_run_device_pyramid_through_a_cycle_equals_run_instagraal(tmp_path):
    from instagraal_amd import pyramid_device, synth
    from instagraal_amd.simulation import run_device_pyramid, run_instagraal

    runs = []
    for k, run in enumerate((run_instagraal, run_device_pyramid)):
        data = str(tmp_path / ("run%d" % k) / "data")  # (the same name: the outputs carry it)
        os.makedirs(os.path.dirname(data))
        synth.write_text_dataset(data, n_contigs=10, mean_frags=110, seed=7, contacts_per_frag=40)
        out = str(tmp_path / ("out%d" % k))
        np.random.seed(17)
        if k == 1:  # the levels are the device's: the run behind them finds every one present and builds none
            made = []
            real = pyramid_device.write_contacts
            pyramid_device.write_contacts = lambda path, data3: (made.append(path), real(path, data3))[1]
        try:
            p2 = run(data, os.path.join(data, "genome.fa"), output_folder=out, level=2, cycles=1, bomb=True)
        finally:
            if k == 1:
                pyramid_device.write_contacts = real
        p2.simulation.release()
        runs.append(out)
    assert len(made) == 9
    a, b = same_tree(runs[0], runs[1]), same_tree(runs[1], runs[0])
    assert sorted(a) == sorted(b) and any(n.endswith("info_frags.txt") for n in a) and any(n.endswith("genome.fasta") for n in a)
    assert sum("abs_frag_contacts" in n for n in a) == 10
