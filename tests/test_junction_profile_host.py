"""CPU tests of the junction support profile's rule (instagraal_amd.junction_profile): ``observed`` against the matrix the
reference's own ``display_current_matrix`` produced on the two ``tiny`` trajectories (tests/golden/matrix_tiny_*.npz), with contig
extents and positions from the oracle's tables on the fixture's state; hand-made tables with a ring, an unplaced contig and a
contig of one sub-fragment; the identities; the closed form of the pairs; the arguments; the import.  Every comparison is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

FIXTURES = ("matrix_tiny_plain", "matrix_tiny_bomb")
WINDOWS = (1, 5, 64, 1024)


def _toy_model_q(s):
    """a stand-in for the quantised model: any deterministic s -> int64 will do for the rule"""
    return np.rint(1000.0 / (1.0 + np.asarray(s, np.float64)) * 2.0 ** 20).astype(np.int64)


@pytest.mark.parametrize("name", FIXTURES)
def test_observed_is_the_reference_matrix_summed_across_every_junction(name, oracle_lib):
    from instagraal_amd import junction_profile as jp, synth
    from oracle.sampler_oracle import OracleSampler

    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    prob = synth.make_problem(*synth.CONFIGS[str(g["config"])])
    state = g["state"]
    s = OracleSampler(**prob.sampler_kwargs(), mode=oracle_lib.MODE_DET)
    s.gpu_vect_frags.assign(oracle_lib.FragStruct(prob.n_frags, {k: state[i] for i, k in enumerate(oracle_lib.FRAG_FIELDS)}))
    s.fill_dist_single()
    dist, stot, contig = s.vect_dist.copy(), s.vect_s_tot.copy(), s.vect_id_c.astype(np.int64)
    order = g["full_order_high"].astype(np.int64)
    matrix = g["matrix"].astype(np.int64)  # (m + m.T)[order][:, order], from the reference
    T = order.size
    assert T == prob.n_sub_frags and np.array_equal(np.sort(order), np.arange(T)) and not stot.any()
    position = np.empty(T, np.int64)
    position[order] = np.arange(T)
    placed = np.ones(T, bool)
    # the genome order walks every contig by the oracle's rank: positions inside a contig are its ranks in a row
    c_pos = contig[order]
    starts = np.concatenate([[0], np.nonzero(c_pos[1:] != c_pos[:-1])[0] + 1])
    assert np.array_equal(s.vect_pos[order], np.arange(T) - np.repeat(starts, np.diff(np.concatenate([starts, [T]]))))
    a, b = np.triu_indices(T, k=1)
    same = c_pos[a] == c_pos[b]
    total = int(matrix[a, b].sum())
    assert total == int(prob.coo_cnt.astype(np.int64).sum())
    internal = np.concatenate([[False], c_pos[1:] == c_pos[:-1]])
    for w in WINDOWS:
        got = jp.profile_host(dist, stot, contig, placed, position, prob.coo_row, prob.coo_col, prob.coo_cnt, w, model_q=_toy_model_q)
        keep = same & (b - a <= w)
        S = np.zeros((T, T), np.int64)
        S[a[keep], b[keep]] = matrix[a[keep], b[keep]]
        R = S.cumsum(0).cumsum(1)  # R[x, y] = sum of S[:x + 1, :y + 1]
        want = np.zeros(T, np.int64)
        j = np.arange(1, T)
        want[1:] = R[j - 1, T - 1] - R[j - 1, j - 1]  # rows a < j, columns b >= j
        assert got["observed"].dtype == np.int64 and np.array_equal(got["observed"], want), w
        assert not got["observed"][~internal].any() and got["observed"][internal].any()
        assert got["in_window_observed"] == int(matrix[a, b][keep].sum())
        assert got["beyond_window_observed"] == int(matrix[a, b][same & ~keep].sum())
        assert got["trans_observed"] == int(matrix[a, b][~same].sum())
        assert got["ring_observed"] == got["unplaced_observed"] == 0 and jp.observed_total(got) == total
        assert got["internal_junctions"] == int(internal.sum()) and got["n_placed"] == T
        assert got["spanned_observed"] == int(want.sum()) == int((matrix[a, b] * (b - a))[keep].sum())
        # the pairs: the band of the same-contig mask, summed the same way
        P = np.zeros((T, T), np.int64)
        P[a[keep], b[keep]] = 1
        RP = P.cumsum(0).cumsum(1)
        want_pairs = np.zeros(T, np.int64)
        want_pairs[1:] = RP[j - 1, T - 1] - RP[j - 1, j - 1]
        assert np.array_equal(got["pairs"], want_pairs), w
        Q = np.zeros((T, T), np.int64)
        Q[a[keep], b[keep]] = _toy_model_q(np.abs(dist[order[a[keep]]] - dist[order[b[keep]]]))
        RQ = Q.cumsum(0).cumsum(1)
        assert np.array_equal(got["expected_q"][1:], RQ[j - 1, T - 1] - RQ[j - 1, j - 1]), w


def _hand_made(seed=0):
    """tables made by hand, in genome order: a ring, a contig that is not placed, a contig of one sub-fragment, two plain ones;
    contacts between everything; the table itself is shuffled"""
    rng = np.random.RandomState(seed)
    lens = [40, 25, 30, 1, 60]
    contig = np.repeat(np.arange(5) * 7 + 3, lens)  # (ids with gaps)
    M = contig.size
    dist = np.concatenate([np.cumsum(rng.uniform(0.2, 3.0, n)) for n in lens]).astype(np.float32)
    stot = np.where(contig == 3, np.float32(77.0), np.float32(0.0)).astype(np.float32)  # the first is a ring
    placed = contig != 10  # the second is not placed
    position = np.where(placed, np.cumsum(placed) - 1, -1)
    perm = rng.permutation(M)
    dist, stot, contig, placed, position = dist[perm], stot[perm], contig[perm], placed[perm], position[perm]
    iu, ju = np.triu_indices(M, k=1)
    keep = rng.rand(iu.size) < 0.3
    row, col = iu[keep], ju[keep]
    cnt = rng.randint(1, 50, row.size)
    return dist, stot, contig, placed, position, row, col, cnt, lens


def _brute(dist, stot, contig, placed, position, row, col, cnt, w, model_q):
    """the definition, pair by pair"""
    T = int(placed.sum())
    where = np.full(T, -1, np.int64)
    where[position[placed]] = np.nonzero(placed)[0]
    obs, prs, exq = np.zeros(T, np.int64), np.zeros(T, np.int64), np.zeros(T, np.int64)
    for r, c, v in zip(row.tolist(), col.tolist(), cnt.tolist()):
        if placed[r] and placed[c] and contig[r] == contig[c] and stot[r] == 0:
            pa, pb = sorted((int(position[r]), int(position[c])))
            if pb - pa <= w:
                obs[pa + 1:pb + 1] += v
    for i in range(T):
        for k in range(i + 1, min(i + w, T - 1) + 1):
            si, sk = where[i], where[k]
            if contig[si] == contig[sk] and stot[si] == 0:
                prs[i + 1:k + 1] += 1
                exq[i + 1:k + 1] += int(model_q(np.abs(dist[si:si + 1] - dist[sk:sk + 1]))[0])
    return obs, prs, exq


@pytest.mark.parametrize("w", [1, 2, 7, 29, 30, 59, 60, 64, 1024])
def test_hand_made_tables_with_a_ring_an_unplaced_contig_and_a_contig_of_one(w):
    from instagraal_amd import junction_profile as jp

    dist, stot, contig, placed, position, row, col, cnt, lens = _hand_made()
    got = jp.profile_host(dist, stot, contig, placed, position, row, col, cnt, w, model_q=_toy_model_q)
    T = int(placed.sum())
    assert all(got[k].dtype == np.int64 and got[k].size == T for k in ("observed", "pairs", "expected_q")) and got["n_placed"] == T
    obs, prs, exq = _brute(dist, stot, contig, placed, position, row, col, cnt, w, _toy_model_q)
    assert np.array_equal(got["observed"], obs) and np.array_equal(got["pairs"], prs) and np.array_equal(got["expected_q"], exq)
    # the three identities
    assert jp.observed_total(got) == int(cnt.sum())
    assert got["ring_observed"] > 0 and got["unplaced_observed"] > 0 and got["trans_observed"] > 0 and got["in_window_observed"] > 0
    lin = placed[row] & placed[col] & (contig[row] == contig[col]) & (stot[row] == 0)
    span = np.abs(position[row] - position[col])
    near = lin & (span <= w)
    assert got["in_window_observed"] == int(cnt[near].sum()) and got["beyond_window_observed"] == int(cnt[lin & ~near].sum())
    assert got["spanned_observed"] == int(got["observed"].sum()) == int((cnt * span)[near].sum())
    linear_lengths = [30, 1, 60]
    assert int(got["pairs"].sum()) == jp.pairs_total_closed_form(linear_lengths, w)
    assert got["internal_junctions"] == sum(n - 1 for n in linear_lengths)
    # ring and boundary junctions are 0, the kinds say which is which
    kind = jp.junction_kinds(stot, contig, position)
    want_kind = np.concatenate([[jp.KIND_BOUNDARY] + [jp.KIND_RING] * 39, [jp.KIND_BOUNDARY] + [jp.KIND_INTERNAL] * 29, [jp.KIND_BOUNDARY],
                                [jp.KIND_BOUNDARY] + [jp.KIND_INTERNAL] * 59])
    assert np.array_equal(kind, want_kind)
    for k in ("observed", "pairs", "expected_q"):
        assert not got[k][kind != jp.KIND_INTERNAL].any() and got[k][kind == jp.KIND_INTERNAL].any()
    assert got["pairs"][kind == jp.KIND_INTERNAL].all() and got["expected_q"][kind == jp.KIND_INTERNAL].all()
    # pairs by the closed form from the local rank, the contig's length and w
    start = np.concatenate([[0], np.nonzero(np.diff(contig[np.argsort(np.where(placed, position, 10 ** 6))][:T]))[0] + 1])
    length = np.diff(np.concatenate([start, [T]]))
    rank = np.arange(T) - np.repeat(start, length)
    closed = np.where(kind == jp.KIND_INTERNAL, jp.pairs_closed_form(rank, np.repeat(length, length), w), 0)
    assert np.array_equal(got["pairs"], closed)
    # a window longer than every contig is the longest window
    if w >= 60:
        far = jp.profile_host(dist, stot, contig, placed, position, row, col, cnt, 1024, model_q=_toy_model_q)
        assert all(np.array_equal(far[k], got[k]) for k in ("observed", "pairs", "expected_q")) and far["beyond_window_observed"] == 0
    # without a model: the same, less expected_q
    lean = jp.profile_host(dist, stot, contig, placed, position, row, col, cnt, w)
    assert lean["expected_q"] is None and np.array_equal(lean["observed"], got["observed"]) and np.array_equal(lean["pairs"], got["pairs"])
    # the chunking of the expansion does not show
    small = jp.profile_host(dist, stot, contig, placed, position, row, col, cnt, w, chunk=64)
    assert np.array_equal(small["observed"], got["observed"])


def test_arguments_are_checked():
    from instagraal_amd import junction_profile as jp

    for bad in (0, 1025, -3, 2.5):
        with pytest.raises(ValueError):
            jp.check_window(bad)
    assert jp.check_window(1) == 1 and jp.check_window(1024) == jp.MAX_WINDOW and jp.check_window(np.int32(64)) == 64
    assert jp.window_from_kb(100.0, 1.6) == 63 and jp.window_from_kb(0.1, 1.6) == 1 and jp.window_from_kb(3.2, 1.6) == 2
    for kb, mean in ((0.0, 1.0), (1.0, 0.0), (np.nan, 1.0), (1.0, np.inf)):
        with pytest.raises(ValueError):
            jp.window_from_kb(kb, mean)
    dist, stot, contig, placed, position, row, col, cnt, _ = _hand_made()
    with pytest.raises(ValueError, match="window"):
        jp.profile_host(dist, stot, contig, placed, position, row, col, cnt, 0)
    with pytest.raises(ValueError, match="disagree"):
        jp.profile_host(dist, stot, contig, ~placed, position, row, col, cnt, 5)
    twice = position.copy()
    twice[np.nonzero(position == 3)[0]] = 4
    with pytest.raises(ValueError, match="each once"):
        jp.profile_host(dist, stot, contig, placed, twice, row, col, cnt, 5)
    swapped = position.copy()  # a sub-fragment of the last contig in the middle of another
    i, k = np.nonzero(position == 45)[0][0], np.nonzero(position == 100)[0][0]
    swapped[i], swapped[k] = 100, 45
    with pytest.raises(ValueError, match="contiguous"):
        jp.profile_host(dist, stot, contig, placed, swapped, row, col, cnt, 5)
    assert jp.default_min_pairs(64) == 1040 and jp.default_min_pairs(1) == 1


def test_ratio_table_and_file(tmp_path):
    from instagraal_amd import junction_profile as jp

    dist, stot, contig, placed, position, row, col, cnt, _ = _hand_made(1)
    prof = jp.profile_host(dist, stot, contig, placed, position, row, col, cnt, 8, model_q=_toy_model_q)
    r = jp.ratio(prof)
    ok = prof["expected_q"] != 0
    assert np.array_equal(r[ok], prof["observed"][ok] / (prof["expected_q"][ok] / 2.0 ** 32)) and np.all(np.isnan(r[~ok]))
    kind = jp.junction_kinds(stot, contig, position)
    T = prof["n_placed"]
    parent = np.arange(T) // 3 + 500  # three sub-fragments per bin
    cpos = contig[np.argsort(np.where(placed, position, 10 ** 6))][:T]
    table = jp.bin_table(prof, kind, parent, cpos)
    j = table["position"]
    assert j.size and np.all(kind[j] == jp.KIND_INTERNAL) and np.all(parent[j] != parent[j - 1])
    assert j.size == int(((kind[1:] == jp.KIND_INTERNAL) & (parent[1:] != parent[:-1])).sum())
    assert np.array_equal(table["left_frag"], parent[j - 1]) and np.array_equal(table["right_frag"], parent[j]) and np.array_equal(table["contig"], cpos[j])
    assert np.array_equal(table["observed"], prof["observed"][j]) and np.array_equal(table["pairs"], prof["pairs"][j])
    weak = jp.weakest(table, 5, min_pairs=jp.default_min_pairs(8))
    assert 0 < weak.size <= 5 and np.all(np.diff(weak["ratio"]) >= 0) and np.all(weak["pairs"] >= 18)
    rest = table[(table["pairs"] >= 18) & ~np.isin(table["position"], weak["position"])]
    assert not rest.size or rest["ratio"].min() >= weak["ratio"].max()
    prof["bins"] = table
    path = str(tmp_path / "junctions.txt")
    jp.write_profile(path, prof)
    t = np.loadtxt(path, ndmin=2)
    assert t.shape == (table.size, len(jp.BIN_COLUMNS))
    for c, k in enumerate(jp.BIN_COLUMNS[:6]):
        assert np.array_equal(t[:, c].astype(np.int64), table[k]), k
    assert np.allclose(t[:, 6], table["expected"], rtol=1e-8) and np.allclose(t[:, 7], table["ratio"], rtol=1e-8)
    trailer = dict(kv.split("=") for kv in open(path).read().splitlines()[-1][2:].split())
    assert int(trailer["window"]) == 8 and all(int(trailer[k]) == prof[k] for k in jp.SCALARS)


def test_import_needs_neither_matplotlib_nor_the_library():
    code = ("import sys; import numpy as np\n"
            "import instagraal_amd.junction_profile as j, instagraal_amd.sampler, instagraal_amd.simulation, instagraal_amd.hip_lib as h\n"
            "p = j.profile_host(np.arange(4, dtype=np.float32), np.zeros(4), np.zeros(4), np.ones(4, bool), np.arange(4), [0, 1], [2, 2], [3, 5], 2)\n"
            "assert p['observed'].tolist() == [0, 3, 8, 0] and p['pairs'].tolist() == [0, 2, 3, 2] and p['expected_q'] is None\n"
            "assert h._lib is None, 'the shared library was loaded'\n"
            "sys.exit(1 if any(m == 'matplotlib' or m.startswith('matplotlib.') for m in sys.modules) else 0)")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
