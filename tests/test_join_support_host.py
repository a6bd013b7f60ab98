"""CPU tests of the join support's rule (instagraal_amd.join_support): the rule against brute force on ``tiny`` -- the dense symmetric
matrix permuted by the genome order, and for every pair of ends the corner triangle depth + depth + 1 <= w summed --, the closed form
of the pairs, the identities, the merge of two shards, the ranking and the file; and that the states the GPU tests use exercise
what they are there for.  Every comparison is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

WINDOWS = (1, 2, 64, 1024)


def _toy_model_q(s):
    """a stand-in for the quantised model: any deterministic s -> int64 will do for the rule"""
    return np.rint(1000.0 / (1.0 + np.asarray(s, np.float64)) * 2.0 ** 20).astype(np.int64)


def _tiny():
    from instagraal_amd import synth

    return synth.make_problem(*synth.CONFIGS["tiny"])


def _tables(prob, seed=None, ring=False, unplaced=False, single=False, nothing=False):
    """a genome made from the problem's contigs: in the table's order (seed None) or the contigs permuted and flipped at random;
    ``ring``: the second contig is a ring; ``unplaced``: the third is not placed; ``single``: the last sub-fragment of the first
    contig is a contig of its own.  -> dist, stot, contig, placed, position, l_cont_bp (per sub-fragment)"""
    parent = prob.np_sub_frags_2_frags["x"].astype(np.int64)
    contig = np.asarray(prob.S_o_A_frags["id_c"], np.int64)[parent].copy()
    ids = np.unique(contig)
    if single:
        contig[np.nonzero(contig == ids[0])[0][-1]] = ids.max() + 1
    ids = np.unique(contig)
    M = contig.size
    len_bp = np.asarray(prob.S_o_A_sub_frags["len_bp"], np.int64)
    rng = np.random.RandomState(seed if seed is not None else 0)
    walk = rng.permutation(ids) if seed is not None else ids
    dist, stot, placed = np.zeros(M, np.float32), np.zeros(M, np.float32), np.ones(M, bool)
    position, l_cont_bp = np.full(M, -1, np.int64), np.zeros(M, np.int64)
    at = 0
    for c in walk.tolist():
        members = np.nonzero(contig == c)[0]
        if seed is not None and rng.rand() < 0.5:
            members = members[::-1]
        bp = np.cumsum(len_bp[members])
        dist[members] = ((bp - len_bp[members]) / 1000.0).astype(np.float32)
        l_cont_bp[members] = bp[-1]
        if ring and c == ids[1]:
            stot[members] = np.float32(bp[-1] / 1000.0)
        if nothing or (unplaced and c == ids[2]):
            placed[members] = False
            continue
        position[members] = at + np.arange(members.size)
        at += members.size
    return dist, stot, contig, placed, position, l_cont_bp


def _brute(prob, dist, stot, contig, placed, position, l_cont_bp, row, col, cnt, w, model_q):
    """the definition on the dense matrix: -> {(lo, hi): (observed, pairs, expected_q)} for every pair of ends of two different
    linear placed contigs, and the contigs' (start, n)"""
    M = dist.size
    D = np.zeros((M, M), np.int64)
    np.add.at(D, (row, col), cnt)
    D = D + D.T
    order = np.nonzero(placed)[0]
    order = order[np.argsort(position[order])]
    Dp = D[order][:, order]
    c_pos = contig[order]
    T = order.size
    starts = np.concatenate([[0], np.nonzero(c_pos[1:] != c_pos[:-1])[0] + 1]) if T else np.zeros(0, np.int64)
    lens = np.diff(np.concatenate([starts, [T]])) if T else np.zeros(0, np.int64)
    lin = [(int(s), int(n)) for s, n in zip(starts, lens) if stot[order[s]] == 0]
    out = {}
    for ka, (sa0, na) in enumerate(lin):
        for kb, (sb0, nb) in enumerate(lin):
            if kb <= ka:
                continue
            for sa in (0, 1):
                for sb in (0, 1):
                    ia = np.arange(sa0, sa0 + na) if sa == 0 else np.arange(sa0 + na - 1, sa0 - 1, -1)
                    ib = np.arange(sb0, sb0 + nb) if sb == 0 else np.arange(sb0 + nb - 1, sb0 - 1, -1)
                    ia, ib = ia[:w], ib[:w]
                    m = np.arange(ia.size)[:, None] + np.arange(ib.size)[None, :] + 1 <= w
                    obs = int(Dp[np.ix_(ia, ib)][m].sum())
                    la = np.float32(l_cont_bp[order[sa0]]) / np.float32(1000.0)
                    lb = np.float32(l_cont_bp[order[sb0]]) / np.float32(1000.0)
                    da = dist[order[ia]] if sa == 0 else np.abs(la - dist[order[ia]])
                    db = dist[order[ib]] if sb == 0 else np.abs(lb - dist[order[ib]])
                    s = (da[:, None] + db[None, :])[m]
                    assert s.dtype == np.float32
                    out[(2 * ka + sa, 2 * kb + sb)] = (obs, int(m.sum()), int(model_q(s).sum()))
    return out, lin


def _as_dict(res):
    from instagraal_amd import join_support as js

    lo = js.rows_of(res["rowptr"])
    return {(int(a), int(b)): (int(o), int(p), int(q)) for a, b, o, p, q in zip(lo, res["col"], res["observed"], res["pairs"], res["expected_q"])}


STATES = dict(fresh={}, shuffled=dict(seed=5), ring=dict(seed=6, ring=True), unplaced=dict(seed=7, unplaced=True), single=dict(seed=8, single=True),
              all_of_it=dict(seed=9, ring=True, unplaced=True, single=True), nothing=dict(nothing=True))


@pytest.mark.parametrize("state", sorted(STATES))
def test_the_rule_equals_brute_force_on_tiny(state):
    from instagraal_amd import join_support as js

    prob = _tiny()
    t = _tables(prob, **STATES[state])
    dist, stot, contig, placed, position, l_cont_bp = t
    row, col, cnt = prob.coo_row.astype(np.int64), prob.coo_col.astype(np.int64), prob.coo_cnt.astype(np.int64)
    total = int(cnt.sum())
    for w in WINDOWS:
        got = js.support_host(*t, row, col, cnt, w, model_q=_toy_model_q)
        want, lin = _brute(prob, *t, row, col, cnt, w, _toy_model_q)
        K = len(lin)
        assert got["n_contigs"] == K and got["rowptr"].dtype == np.int64 and got["rowptr"].size == 2 * K + 1 and got["col"].dtype == np.int32
        assert got["first_position"].tolist() == [s for s, _ in lin] and got["n_positions"].tolist() == [n for _, n in lin]
        assert _as_dict(got) == {k: v for k, v in want.items() if v[0] > 0}, (state, w)
        assert got["n_links"] == got["col"].size == int(got["rowptr"][-1])
        lo = js.rows_of(got["rowptr"])
        assert np.all(lo < got["col"]) and np.all(lo >> 1 != got["col"] >> 1)  # never two ends of one contig
        for r in range(2 * K):  # strictly ascending inside a row
            assert np.all(np.diff(got["col"][got["rowptr"][r]:got["rowptr"][r + 1]]) > 0)
        # the identities
        assert js.observed_total(got) == total and int(got["observed"].sum()) == got["contributions"]
        n = [n for _, n in lin]
        if K >= 2 and w >= sorted(n)[-1] + sorted(n)[-2] - 1:
            assert got["out_of_reach_observed"] == 0 and got["contributions"] == 4 * got["in_reach_observed"]
        if w == 1:
            D = np.zeros((dist.size, dist.size), np.int64)
            np.add.at(D, (row, col), cnt)
            D = D + D.T
            order = np.nonzero(placed)[0][np.argsort(position[placed])]
            end_frag = lambda e: order[lin[e >> 1][0] + (lin[e >> 1][1] - 1) * (e & 1)]  # noqa: E731
            assert np.all(got["pairs"] == 1)
            assert all(o == D[end_frag(a), end_frag(b)] for (a, b), (o, _, _) in _as_dict(got).items())
        assert np.array_equal(got["pairs"], js.pairs_closed_form(got["n_positions"][lo >> 1], got["n_positions"][got["col"] >> 1], w))
        if state == "nothing":
            assert K == 0 and got["n_links"] == 0 and got["unplaced_observed"] == total and got["rowptr"].tolist() == [0]
        if state == "all_of_it":
            assert got["ring_observed"] > 0 and got["unplaced_observed"] > 0 and got["cis_observed"] > 0 and 1 in n
        if state != "nothing" and w >= 64:
            assert got["in_reach_observed"] > 0 and got["n_links"] > 0
        lean = js.support_host(*t, row, col, cnt, w)  # without a model: the same, less the model part
        assert lean["pairs"] is None and lean["expected_q"] is None and np.array_equal(lean["observed"], got["observed"])
        small = js.support_host(*t, row, col, cnt, w, model_q=_toy_model_q, chunk=50)  # the chunking of the enumeration does not show
        assert all(np.array_equal(small[k], got[k]) for k in js.LINK_ARRAYS)


def test_no_contacts():
    from instagraal_amd import join_support as js

    prob = _tiny()
    none = np.zeros(0, np.int64)
    got = js.support_host(*_tables(prob, seed=3), none, none, none, 64, model_q=_toy_model_q)
    assert got["n_contigs"] == 6 and not got["rowptr"].any() and got["rowptr"].size == 13 and got["n_links"] == 0
    assert all(got[k].size == 0 for k in js.LINK_ARRAYS) and all(got[k] == 0 for k in js.SUMMED_SCALARS)


def test_pairs_closed_form_against_enumeration():
    from instagraal_amd import join_support as js

    for w in (1, 2, 5, 9, 10, 11, 64):
        for na in (1, 2, w - 1, w, w + 1, 2 * w + 3):
            for nb in (1, 2, w - na, w - na + 1, w - na + 2, w - 1, w, w + 1, 3 * w):
                if na < 1 or nb < 1:
                    continue
                want = sum(1 for u in range(min(na, w)) for v in range(min(nb, w)) if u + v + 1 <= w)
                assert js.pairs_closed_form(na, nb, w) == want == sum(min(nb, w - u) for u in range(min(w, na))), (na, nb, w)
    assert js.pairs_closed_form(5000, 5000, 1024) == 1024 * 1025 // 2
    assert js.pairs_closed_form(np.array([3, 3]), np.array([3, 1]), 1024).tolist() == [9, 3]


def test_arguments_are_checked():
    from instagraal_amd import join_support as js, junction_profile as jp

    assert js.MAX_WINDOW is jp.MAX_WINDOW and js.check_window is jp.check_window and js.window_from_kb is jp.window_from_kb
    prob = _tiny()
    t = _tables(prob)
    row, col, cnt = prob.coo_row, prob.coo_col, prob.coo_cnt
    for bad in (0, 1025, 2.5):
        with pytest.raises(ValueError, match="window"):
            js.support_host(*t, row, col, cnt, bad)
    with pytest.raises(ValueError, match="disagree"):
        js.support_host(t[0], t[1], t[2], ~t[3], t[4], t[5], row, col, cnt, 5)
    assert js.default_min_pairs(64) == 1040


def test_the_merge_of_two_shards():
    from instagraal_amd import join_support as js

    prob = _tiny()
    t = _tables(prob, seed=11, ring=True, unplaced=True)
    row, col, cnt = prob.coo_row.astype(np.int64), prob.coo_col.astype(np.int64), prob.coo_cnt.astype(np.int64)
    for w in (2, 64):
        whole = js.support_host(*t, row, col, cnt, w, model_q=_toy_model_q)
        parts = [js.support_host(*t, row[row % 2 == r], col[row % 2 == r], cnt[row % 2 == r], w, model_q=_toy_model_q) for r in range(2)]
        if w == 64:  # links only one part has, and links both have: their observed add up
            keys = [set(zip(js.rows_of(p["rowptr"]).tolist(), p["col"].tolist())) for p in parts]
            assert keys[0] & keys[1] and keys[0] ^ keys[1]
        merged = js.merge_shards(parts)
        assert all(np.array_equal(merged[k], whole[k]) and merged[k].dtype == whole[k].dtype for k in js.LINK_ARRAYS + ("rowptr",))
        assert all(merged[k] == whole[k] for k in js.SCALARS) and merged["window"] == w
        lean = js.merge_shards([dict(p, pairs=None, expected_q=None) for p in parts])
        assert lean["pairs"] is None and np.array_equal(lean["observed"], whole["observed"])
    with pytest.raises(ValueError):
        js.merge_shards([parts[0], dict(parts[1], window=3)])
    with pytest.raises(ValueError):
        js.merge_shards([])


def _hand_made_table():
    """four contigs, eight ends; links (0,2) (0,5) (1,2) (3,4) (3,6) (5,6)"""
    from instagraal_amd import join_support as js

    res = dict(window=4, rowptr=np.array([0, 2, 3, 3, 5, 5, 6, 6, 6], np.int64), col=np.array([2, 5, 2, 4, 6, 6], np.int32),
               observed=np.array([50, 10, 40, 90, 3, 7], np.int64), pairs=np.array([10, 10, 10, 10, 2, 10], np.int64),
               expected_q=(np.array([10, 10, 10, 10, 1, 0], np.int64) << 32), n_contigs=4, n_links=6)
    res.update({k: 0 for k in js.SCALARS if k not in res})
    res["ends"] = js.ends_table(np.array([0, 5, 9, 10]), np.array([5, 4, 1, 6]), np.arange(16), np.arange(16) // 2, np.array([4, 4, 4, 2, 2, 0, 0, 0]), np.full(16, 100))
    return res


def test_best_joins_and_write_joins_on_a_hand_made_table(tmp_path):
    from instagraal_amd import join_support as js
    from instagraal_amd.assembly_contacts import SCAFFOLD_PREFIX

    res = _hand_made_table()
    assert js.ratio(res)[:5].tolist() == [5.0, 1.0, 4.0, 9.0, 3.0] and np.isnan(js.ratio(res)[5])
    ends = res["ends"]
    assert ends["side"].tolist() == [0, 1] * 4 and ends["sub_frag"].tolist() == [0, 4, 5, 8, 9, 9, 10, 15]
    assert ends["n_positions"].tolist() == [5, 5, 4, 4, 1, 1, 6, 6] and ends["length_bp"].tolist() == [500, 500, 400, 400, 100, 100, 600, 600]
    assert ends["bin"].tolist() == [0, 2, 2, 4, 4, 4, 5, 7] and ends["scaffold"].tolist() == [4, 4, 4, 2, 2, 2, 0, 0]
    best = js.best_joins(res, n=3)  # min_pairs: half of 4 * 5 / 2 = 5: the link of two pairs is out, the one without a ratio too
    assert list(zip(best["end_a"].tolist(), best["end_b"].tolist())) == [(3, 4), (0, 2), (1, 2)] and best["ratio"].tolist() == [9.0, 5.0, 4.0]
    assert best["observed"].tolist() == [90, 50, 40] and best["pairs"].tolist() == [10, 10, 10] and best["expected"].tolist() == [10.0, 10.0, 10.0]
    assert np.isnan(best["runner_up_a"][0]) and np.isnan(best["runner_up_b"][0])  # ends 3 and 4 have no other eligible link
    assert best["runner_up_a"][1] == 1.0 and best["runner_up_b"][1] == 4.0 and np.isnan(best["runner_up_a"][2]) and best["runner_up_b"][2] == 5.0
    everything = js.best_joins(res, n=20, min_pairs=0)
    assert everything.size == 5 and everything["ratio"].tolist() == [9.0, 5.0, 4.0, 3.0, 1.0] and everything["runner_up_a"][0] == 3.0
    assert js.best_joins(res, n=0).size == 0 and js.best_joins(res, min_pairs=10 ** 9).size == 0
    with pytest.raises(ValueError):
        js.best_joins(dict(res, pairs=None))
    path = str(tmp_path / "joins.txt")
    assert js.write_joins(path, res) == 6
    lines = open(path).read().splitlines()
    assert lines[0][2:].split() == list(js.JOIN_COLUMNS) and len(lines) == 8
    rows = [ln.split() for ln in lines[1:-1]]
    assert rows[0] == [SCAFFOLD_PREFIX + "4", "head", SCAFFOLD_PREFIX + "4", "head", "50", "10", "10", "5"]
    assert rows[3][:4] == [SCAFFOLD_PREFIX + "2", "tail", SCAFFOLD_PREFIX + "2", "head"] and rows[5][4:] == ["7", "10", "0", "nan"]
    trailer = dict(kv.split("=") for kv in lines[-1][2:].split())
    assert int(trailer["window"]) == 4 and int(trailer["n_links"]) == 6 and set(js.SCALARS) <= set(trailer)


def _oracle_tables(oracle_lib, prob, state=None, bomb=False):
    """the tables of a state as the device has them, from the oracle: -> what support_host takes"""
    from oracle.sampler_oracle import OracleSampler

    s = OracleSampler(**prob.sampler_kwargs(), mode=oracle_lib.MODE_DET)
    if state is not None:
        s.gpu_vect_frags.assign(oracle_lib.FragStruct(prob.n_frags, {k: state[i] for i, k in enumerate(oracle_lib.FRAG_FIELDS)}))
    if bomb:
        s.bomb_the_genome()
    s.fill_dist_single()
    contig = s.vect_id_c.astype(np.int64)
    order = np.lexsort((s.vect_pos, contig))
    position = np.empty(order.size, np.int64)
    position[order] = np.arange(order.size)
    parent = prob.np_sub_frags_2_frags["x"].astype(np.int64)
    return s.vect_dist.copy(), s.vect_s_tot.copy(), contig, np.ones(order.size, bool), position, np.asarray(s.gpu_vect_frags.l_cont_bp, np.int64)[parent]


@pytest.mark.parametrize("what", ["matrix_tiny_plain", "matrix_tiny_bomb", "small", "small_bombed"])
def test_the_states_of_the_gpu_tests_exercise_the_rule(what, oracle_lib):
    """the states tests/test_hip_join_support.py compares on: contacts in reach, links fed by more than one contact, contacts that count
    for four links, and links on both sides of the model pass's threshold between its two forms (JOIN_WAVE_PAIRS = 66 pairs: the
    full window of 11 positions is the last a thread sums, the full window of 12, 78 pairs, the first a wave does)"""
    from instagraal_amd import join_support as js, synth

    if what.startswith("matrix"):
        g = np.load(os.path.join(GOLDEN, what + ".npz"))
        prob = synth.make_problem(*synth.CONFIGS[str(g["config"])])
        t = _oracle_tables(oracle_lib, prob, state=g["state"])
    else:
        prob = synth.make_problem(*synth.CONFIGS["small"])
        t = _oracle_tables(oracle_lib, prob, bomb=what == "small_bombed")
    row, col, cnt = prob.coo_row.astype(np.int64), prob.coo_col.astype(np.int64), prob.coo_cnt.astype(np.int64)
    pairs_seen = set()
    for w in (1, 10, 11, 12, 63, 64, 65, 1024):
        got = js.support_host(*t, row, col, cnt, w, model_q=_toy_model_q)
        assert js.observed_total(got) == int(cnt.sum()) and int(got["observed"].sum()) == got["contributions"]
        assert got["in_reach_observed"] > 0, (what, w)
        pairs_seen |= set(got["pairs"].tolist())
        if w >= 63:
            assert got["entries"] > got["n_links"] > 0  # links fed by more than one contact
            assert got["contributions"] > got["in_reach_observed"]  # contacts that count for more than one link ...
        if w == 1024:
            n = np.sort(got["n_positions"])
            if n[-1] + n[-2] - 1 <= w:  # ... every one of them for four
                assert got["contributions"] == 4 * got["in_reach_observed"] and got["out_of_reach_observed"] == 0
            else:
                four = (got["n_positions"][:, None] + got["n_positions"][None, :] - 1 <= w) & ~np.eye(n.size, dtype=bool)
                assert four.any()
    if what == "small_bombed":
        assert got["n_contigs"] == prob.n_frags and max(pairs_seen) <= 66
    else:
        assert min(pairs_seen) <= 66 < max(pairs_seen)
    if what == "small":  # full windows of 10, 11 and 12 positions: 55 and 66 pairs (a thread per link), 78 (a wave)
        assert {55, 66, 78} <= pairs_seen and not pairs_seen & set(range(67, 78)), sorted(p for p in pairs_seen if 50 < p < 90)


def test_import_needs_neither_matplotlib_nor_the_library():
    code = ("import sys; import numpy as np\n"
            "import instagraal_amd.join_support as j, instagraal_amd.sampler, instagraal_amd.simulation, instagraal_amd.hip_lib as h\n"
            "r = j.support_host(np.arange(4, dtype=np.float32), np.zeros(4), [0, 0, 1, 1], np.ones(4, bool), np.arange(4), np.full(4, 2000), [0, 1], [2, 3], [3, 5], 1)\n"
            "assert r['rowptr'].tolist() == [0, 1, 2, 2, 2] and r['col'].tolist() == [2, 3] and r['observed'].tolist() == [3, 5] and r['pairs'] is None, r\n"
            "r = j.support_host(np.arange(4, dtype=np.float32), np.zeros(4), [0, 0, 1, 1], np.ones(4, bool), np.arange(4), np.full(4, 2000), [0, 1], [2, 3], [3, 5], 2)\n"
            "assert r['rowptr'].tolist() == [0, 2, 4, 4, 4] and r['col'].tolist() == [2, 3, 2, 3] and r['observed'].tolist() == [3, 8, 8, 5], r\n"
            "assert h._lib is None, 'the shared library was loaded'\n"
            "sys.exit(1 if any(m == 'matplotlib' or m.startswith('matplotlib.') for m in sys.modules) else 0)")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
