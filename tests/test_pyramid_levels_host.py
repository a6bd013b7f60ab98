"""The rule of the pyramid's contact levels (instagraal_amd/pyramid_levels.py) against the host code it restates
(pyramid.fill_sparse_pyramid_level, pyramid._accumulate_contacts, scipy's degrees), and pyramid_device.build_and_filter(device=False)
against pyramid.build_and_filter and the golden of the reference's own builder.  Every comparison is exact.  No GPU."""
import filecmp
import os

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import GOLDEN


def random_list(seed, n_frags, n, zeros=True):
    """a list with a > b, both (a, b) and (b, a), repeats, diagonal entries and zero counts"""
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, n_frags, n), rng.integers(0, n_frags, n)
    k = n // 5
    a[:k], b[:k] = b[k:2 * k].copy(), a[k:2 * k].copy()  # (b, a) of other entries
    a[2 * k:2 * k + k // 2] = b[2 * k:2 * k + k // 2]  # the diagonal
    a[-k:], b[-k:] = a[:k], b[:k]  # repeats
    count = rng.integers(1, 50, n)
    if zeros:
        count[rng.integers(0, n, n // 6)] = 0
    p = rng.permutation(n)
    return a[p].astype(np.int64), b[p].astype(np.int64), count[p].astype(np.int64)


def write_list(path, a, b, count):
    with open(path, "w") as f:
        f.write("id_frag_a\tid_frag_b\tn_contact\n")
        for x, y, c in zip(a.tolist(), b.tolist(), count.tolist()):
            f.write("%d\t%d\t%d\n" % (x, y, c))


class Store:
    def put(self, level, data3, nfrags):
        self.data3, self.nfrags = data3, nfrags


@pytest.mark.parametrize("seed,n_frags,n", [(1, 7, 60), (2, 300, 2000), (3, 1, 5), (4, 50, 0)])
def test_level_matrix_is_the_accumulation_and_for_a_canonical_list_the_filled_level(tmp_path, seed, n_frags, n):
    from instagraal_amd import pyramid, pyramid_levels as rule
    from instagraal_amd.pyramid_device import read_contacts

    a, b, count = random_list(seed, n_frags, n)
    row, col, tot = rule.level_matrix(a, b, count)
    f1, f2, want = pyramid._accumulate_contacts(a, b, count)
    assert np.array_equal(row, f1) and np.array_equal(col, f2) and np.array_equal(tot, want)
    assert rule.canonical(row, col) and (n == 0 or not rule.canonical(a, b))
    # the level is a canonical list, and the reference's fill of it is the level itself; of the raw list, the same sums in another order
    path = str(tmp_path / "c.txt")
    write_list(path, row, col, tot)
    ra, rb, rc = read_contacts(path)
    assert np.array_equal(ra, row) and np.array_equal(rb, col) and np.array_equal(rc, tot)
    s = Store()
    pyramid.fill_sparse_pyramid_level(s, 0, path, n_frags)
    assert np.array_equal(s.data3, rule.data3((row, col, tot))) and s.data3.dtype == np.int32
    write_list(path, a, b, count)
    pyramid.fill_sparse_pyramid_level(s, 0, path, n_frags)
    order = np.lexsort((s.data3[1], s.data3[0]))
    assert np.array_equal(s.data3[:, order], rule.data3((row, col, tot)))
    again = rule.level_matrix(row, col, tot)
    assert all(np.array_equal(x, y) for x, y in zip(again, (row, col, tot)))  # the device result for a canonical list is the list


def test_canonical_on_and_off():
    from instagraal_amd.pyramid_levels import canonical

    assert canonical([], []) and canonical([3], [3]) and canonical([0, 0, 1, 2], [0, 5, 1, 2])
    assert not canonical([1], [0])  # a > b
    assert not canonical([0, 0], [2, 2])  # a repeat
    assert not canonical([0, 0], [3, 2])  # columns descending
    assert not canonical([1, 0], [2, 3])  # rows descending
    assert canonical([0, 1], [9, 1])


@pytest.mark.parametrize("seed,n_frags,n", [(5, 9, 80), (6, 400, 3000)])
def test_degrees_are_scipys(seed, n_frags, n):
    from instagraal_amd import pyramid_levels as rule

    a, b, count = random_list(seed, n_frags, n)
    M = rule.level_matrix(a, b, count)
    assert (M[2] == 0).any() and (M[0] == M[1]).any()
    d3 = rule.data3(M)
    csr = sp.csr_matrix((d3[2, :], d3[0:2, :]), shape=(n_frags, n_frags))
    full = csr + csr.transpose()
    assert np.array_equal(rule.degrees(M, n_frags), np.diff(full.indptr))


def test_remap_drops_the_first_entry_in_file_order_and_the_destroyed_fragments():
    from instagraal_amd import pyramid, pyramid_levels as rule

    a, b, count = random_list(7, 40, 500, zeros=False)
    a[0], b[0], count[0] = 39, 2, 1000  # the first entry in file order is far from the first in sorted order
    lut = np.arange(40) // 3
    lut[[4, 5, 17, 39]] = -1
    for skip in (False, True):
        sc = {}
        row, col, tot = rule.remap(a, b, count, lut, skip, scalars=sc)
        x, y, c = (v[1:] for v in (a, b, count)) if skip else (a, b, count)
        keep = (lut[x] >= 0) & (lut[y] >= 0)
        f1, f2, want = pyramid._accumulate_contacts(lut[x][keep], lut[y][keep], c[keep])
        assert np.array_equal(row, f1) and np.array_equal(col, f2) and np.array_equal(tot, want)
        assert sc["entries_in"] == 500 and sc["skipped"] == int(skip) and sc["dropped_by_lut"] == int((~keep).sum()) and sc["pixels"] == row.size
        assert sc["entries_kept"] + sc["dropped_by_lut"] + sc["skipped"] == 500 and sc["largest_sum"] == int(tot.max())
    # the sorted order's first entry is (0, ...): dropping IT would give another level
    lut2 = np.arange(40)
    with_first = rule.remap(a, b, count, lut2, False)
    without = rule.remap(a, b, count, lut2, True)
    k = np.nonzero((with_first[0] == 2) & (with_first[1] == 39))[0][0]
    assert with_first[2].sum() - without[2].sum() == 1000 and with_first[2][k] >= 1000
    assert rule.remap(a[:1], b[:1], count[:1], lut2, True)[0].size == 0 and rule.remap(a[:0], b[:0], count[:0], lut2, True)[0].size == 0


def test_a_sum_of_2_to_the_31_is_refused_and_one_less_passes():
    from instagraal_amd import pyramid_levels as rule

    top = (1 << 31) - 1
    a, b = np.array([3, 5, 5, 3]), np.array([5, 3, 5, 5])
    row, col, tot = rule.level_matrix(a, b, np.array([top - 10, 4, 7, 6]))
    assert tot.tolist() == [top, 7]
    with pytest.raises(rule.LevelOverflow, match=r"level 4: the sum of the pixel \(3, 5\) is 2147483648"):
        rule.level_matrix(a, b, np.array([top - 10, 5, 7, 6]), level=4)
    with pytest.raises(rule.LevelOverflow, match=r"\(0, 1\)"):
        rule.remap(a, b, np.array([top, 1, 0, 0]), np.array([0, 0, 0, 0, 0, 1]), False, level=2)
    assert rule.remap(a, b, np.array([top, 1, 0, 0]), np.array([0, 0, 0, 0, 0, 1]), True)[2].tolist() == [1, 0]
    with pytest.raises(rule.LevelOverflow):  # sums that would wrap an int64 are refused, not wrapped
        rule.level_matrix(np.zeros(4, np.int64), np.zeros(4, np.int64), np.full(4, (1 << 62)))


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    from instagraal_amd import pyramid, pyramid_device, synth

    g = np.load(os.path.join(GOLDEN, "pyramid_small.npz"))
    work = tmp_path_factory.mktemp("pyrlev")
    data, host, rule_out = str(work / "data"), str(work / "host"), str(work / "rule")
    nc, mf, seed, cpf = [int(x) for x in g["dataset"]]
    synth.write_text_dataset(data, n_contigs=nc, mean_frags=mf, seed=seed, contacts_per_frag=cpf)
    os.makedirs(host), os.makedirs(rule_out)
    p_host = pyramid.build_and_filter(data, 9, 3, thresh_factor=1, output_folder=host)
    p_rule = pyramid_device.build_and_filter(data, 9, 3, thresh_factor=1, output_folder=rule_out, device=False)
    return g, data, host, rule_out, p_host, p_rule


def same_tree(x, y):
    """every file of x is in y with the same bytes and the other way round (the stores apart: compared as arrays)"""
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


def test_the_rule_path_writes_the_host_paths_folders_and_the_goldens(built):
    from instagraal_amd import pyramid, pyramid_levels as rule
    from instagraal_amd.pyramid_device import read_contacts

    g, data, host, rule_out, p_host, p_rule = built
    a = same_tree(os.path.join(host, "pyramids"), os.path.join(rule_out, "pyramids"))
    b = same_tree(os.path.join(rule_out, "pyramids"), os.path.join(host, "pyramids"))
    assert sorted(a) == sorted(b) and len(a) == 9 * 4 - 1 + 3  # (the last level has no index file)
    root = os.path.join(rule_out, "pyramids")
    for rel in g["txt_names"]:
        assert open(os.path.join(root, str(rel)), "rb").read() == g["txt/" + str(rel)].tobytes(), rel
    for lv in range(9):
        d, n = p_rule.store.get(lv)
        dh, nh = p_host.store.get(lv)
        assert n == nh == int(g["h5/%d/nfrags" % lv][0, 0]) and np.array_equal(d, dh) and np.array_equal(d, g["h5/%d/data" % lv]), lv
        assert d.dtype == np.int32
    s_rule, s_host = pyramid.SparseStore(os.path.join(root, "pyramid_1_no_thresh")), pyramid.SparseStore(os.path.join(host, "pyramids", "pyramid_1_no_thresh"))
    assert np.array_equal(s_rule.get(0)[0], s_host.get(0)[0]) and s_rule.get(0)[1] == s_host.get(0)[1]
    # what the golden's dataset covers: the map to -1, a canonical level-0 list, the dropped first line at levels 4 - 8
    la, lb, lc = read_contacts(os.path.join(data, "abs_fragments_contacts_weighted.txt"))
    assert rule.canonical(la, lb)
    n0, n1 = s_host.get(0)[1], p_host.store.get(0)[1]
    assert (n0, n1) == (1095, 1036)
    visible = []
    for lv in range(8):
        x, y, c = read_contacts(os.path.join(root, "pyramid_9_thresh_auto", "level_%d" % lv, "%d_abs_frag_contacts.txt" % lv))
        sup = p_host.spec_level[str(lv)]["super_index"] - 1
        kept, lost = rule.remap(x, y, c, sup, True), rule.remap(x, y, c, sup, False)
        if kept[0].size != lost[0].size or not np.array_equal(kept[2], lost[2]):
            visible.append(lv + 1)
        assert np.array_equal(rule.data3(kept), p_host.store.get(lv + 1)[0])
    assert set(visible) >= {4, 5, 6, 7, 8}  # Q-P1 shows where the first pixel is not summed with another one
    for lv in (3, 4):  # the loader on both: the same arrays, the mean trans level included
        x, y = p_rule.get_level(lv), p_host.get_level(lv)
        assert float(x.mean_value_trans) == float(y.mean_value_trans) and x.n_frags == y.n_frags
    assert float(p_rule.get_level(int(g["level"])).mean_value_trans) == float(g["level/mean_value_trans"])


def test_a_second_call_reuses_every_level_and_a_missing_one_is_made_again(built, tmp_path):
    from instagraal_amd import pyramid_device

    g, data, host, rule_out, p_host, p_rule = built
    root = os.path.join(rule_out, "pyramids", "pyramid_9_thresh_auto")
    stamp = {f: os.path.getmtime(os.path.join(b, f)) for b, _, fs in os.walk(root) for f in fs if f.endswith(".txt")}
    chain = pyramid_device.Chain(False)
    pyramid_device.build_and_filter(data, 9, 3, thresh_factor=1, output_folder=rule_out, device=False, _chain=chain).close()
    assert chain.engine is None and chain.seconds["device"] == 0.0  # nothing was read, nothing was made
    assert stamp == {f: os.path.getmtime(os.path.join(b, f)) for b, _, fs in os.walk(root) for f in fs if f.endswith(".txt")}
    victim = os.path.join(root, "level_5", "5_abs_frag_contacts.txt")
    want = open(victim, "rb").read()
    os.remove(victim)
    pyramid_device.build_and_filter(data, 9, 3, thresh_factor=1, output_folder=rule_out, device=False).close()
    assert open(victim, "rb").read() == want


def test_level0_in_memory_and_a_list_that_is_not_canonical(tmp_path):
    """a shuffled input list with both orders of a pair: build() (where level 1 loses the first entry IN FILE ORDER) and
    build_and_filter through the rule equal the host path; level0 handed over in memory gives the same folders"""
    import shutil

    from instagraal_amd import pyramid, pyramid_device, synth
    from instagraal_amd.pyramid_device import read_contacts

    data = str(tmp_path / "data")
    synth.write_text_dataset(data, n_contigs=5, mean_frags=40, seed=11, contacts_per_frag=6)
    path = os.path.join(data, "abs_fragments_contacts_weighted.txt")
    a, b, c = read_contacts(path)
    rng = np.random.default_rng(3)
    p = rng.permutation(a.size)
    a, b, c = a[p], b[p], c[p]
    flip = rng.random(a.size) < 0.5
    a, b = np.where(flip, b, a), np.where(flip, a, b)
    a, b, c = np.concatenate((a, b[:50])), np.concatenate((b, a[:50])), np.concatenate((c, c[:50]))
    write_list(path, a, b, c)
    outs = {k: str(tmp_path / k) for k in ("host", "rule", "mem")}
    for o in outs.values():
        os.makedirs(o)
    for mbc in (1, 4):
        pyramid.build(data, 3, 3, mbc, output_folder=outs["host"])
        pyramid_device.build(data, 3, 3, mbc, output_folder=outs["rule"], device=False)
        pyramid_device.build(data, 3, 3, mbc, output_folder=outs["mem"], device=False, level0=(a, b, c))
        for o in ("rule", "mem"):
            assert same_tree(os.path.join(outs["host"], "pyramids"), os.path.join(outs[o], "pyramids"))
            for lv in range(3):
                f = "pyramid_3_no_thresh"
                got, want = pyramid.SparseStore(os.path.join(outs[o], "pyramids", f)).get(lv), pyramid.SparseStore(os.path.join(outs["host"], "pyramids", f)).get(lv)
                assert np.array_equal(got[0], want[0]) and got[1] == want[1], (o, lv)
        for o in outs.values():
            shutil.rmtree(os.path.join(o, "pyramids"))
    for tf in (0, 1, 3):
        ph = pyramid.build_and_filter(data, 4, 3, thresh_factor=tf, output_folder=outs["host"])
        pm = pyramid_device.build_and_filter(data, 4, 3, thresh_factor=tf, output_folder=outs["mem"], device=False, level0=(a, b, c))
        assert same_tree(os.path.join(outs["host"], "pyramids"), os.path.join(outs["mem"], "pyramids"))
        for lv in range(4):
            assert np.array_equal(ph.store.get(lv)[0], pm.store.get(lv)[0]) and ph.store.get(lv)[1] == pm.store.get(lv)[1], (tf, lv)
        ph.close(), pm.close()
        for o in ("host", "mem"):
            shutil.rmtree(os.path.join(outs[o], "pyramids"))
