"""CPU tests of the orientation support's rule (instagraal_amd.orientation_support): hand-made tables with a ring, an unplaced contig
and a contig of one position against the definition contact by contact; the exact swap of the quadrants under a reversal in place;
the segment builders on the three state situations; ``keep + flip`` against the matrix the reference's own
``display_current_matrix`` produced on the two ``tiny`` trajectories (tests/golden/matrix_tiny_*.npz).  Every comparison is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

FIXTURES = ("matrix_tiny_plain", "matrix_tiny_bomb")


def _toy_model_q(s):
    """a stand-in for the quantised model: any deterministic s -> int64 will do for the rule"""
    return np.rint(1000.0 / (1.0 + np.asarray(s, np.float64)) * 2.0 ** 20).astype(np.int64)


def _hand_made(seed=0):
    """tables made by hand, in genome order: a linear contig of 40 positions, a ring of 25, a contig that is not placed, a contig of
    one position, a linear one of 60; contacts between everything; the table itself is shuffled.  Positions: the 40 at 0 .. 39, the
    ring at 40 .. 64, the one at 65, the 60 at 66 .. 125"""
    rng = np.random.RandomState(seed)
    lens = [40, 25, 30, 1, 60]
    contig = np.repeat(np.arange(5) * 7 + 3, lens)
    M = contig.size
    dist = np.concatenate([np.cumsum(rng.uniform(0.2, 3.0, n)) for n in lens]).astype(np.float32)
    stot = np.where(contig == 10, np.float32(77.0), np.float32(0.0)).astype(np.float32)  # the second is a ring
    placed = contig != 17  # the third is not placed
    position = np.where(placed, np.cumsum(placed) - 1, -1)
    perm = rng.permutation(M)
    dist, stot, contig, placed, position = dist[perm], stot[perm], contig[perm], placed[perm], position[perm]
    iu, ju = np.triu_indices(M, k=1)
    keep = rng.rand(iu.size) < 0.3
    row, col = iu[keep], ju[keep]
    cnt = rng.randint(1, 50, row.size)
    return dist, stot, contig, placed, position, row, col, cnt


# segments on the hand-made tables: at the head of the 40 (no left flank), inside it (3, 2 and 7 positions), one position, at its
# tail (no right flank); two on the ring; the contig of one; the whole 60 would have no flank -- here its head, a long one, its tail
HAND_FIRST = np.array([0, 6, 10, 12, 20, 36, 41, 50, 65, 66, 70, 120])
HAND_LAST = np.array([3, 8, 11, 18, 20, 39, 45, 50, 65, 69, 110, 125])


def _brute(dist, stot, contig, placed, position, row, col, cnt, first, last, geo, w, model_q):
    """the definition, contact by contact and pair by pair, with python loops"""
    T = int(placed.sum())
    where = np.full(T, -1, np.int64)
    where[position[placed]] = np.nonzero(placed)[0]
    seg = np.full(T, -1, np.int64)
    for k, (f, l) in enumerate(zip(first.tolist(), last.tolist())):
        seg[f:l + 1] = k
    obs = np.zeros((first.size, 4), np.int64)
    sc = dict(unplaced=0, trans=0, ring=0, within_segment=0, counted=0, uncounted=0)
    for r, c, v in zip(row.tolist(), col.tolist(), cnt.tolist()):
        if not (placed[r] and placed[c]):
            sc["unplaced"] += v
        elif contig[r] != contig[c]:
            sc["trans"] += v
        elif stot[r] != 0:
            sc["ring"] += v
        else:
            pa, pb = sorted((int(position[r]), int(position[c])))
            sa, sb = int(seg[pa]), int(seg[pb])
            if sa >= 0 and sa == sb:
                sc["within_segment"] += v
                continue
            hit = 0
            if sa >= 0 and geo[sa, 0] == 0 and pb - last[sa] <= w:
                m = int(geo[sa, 1])
                if first[sa] <= pa <= first[sa] + m - 1:
                    obs[sa, 1] += v
                    hit += 1
                elif last[sa] - m + 1 <= pa <= last[sa]:
                    obs[sa, 3] += v
                    hit += 1
            if sb >= 0 and geo[sb, 0] == 0 and first[sb] - pa <= w:
                m = int(geo[sb, 1])
                if first[sb] <= pb <= first[sb] + m - 1:
                    obs[sb, 0] += v
                    hit += 1
                elif last[sb] - m + 1 <= pb <= last[sb]:
                    obs[sb, 2] += v
                    hit += 1
            sc["counted" if hit else "uncounted"] += v
    exq = np.zeros((first.size, 2), np.int64)
    for k in range(first.size):
        if geo[k, 0] != 0:
            continue
        m, lf, rf = (int(x) for x in geo[k, 1:])
        f, l = int(first[k]), int(last[k])
        for arm_left, arm in ((True, range(f, f + m)), (False, range(l - m + 1, l + 1))):
            for flank_left, flank in ((True, range(f - lf, f)), (False, range(l + 1, l + 1 + rf))):
                for i in arm:
                    for j in flank:
                        q = int(model_q(np.abs(dist[where[i]:where[i] + 1] - dist[where[j]:where[j] + 1]))[0])
                        exq[k, 0 if arm_left == flank_left else 1] += q
    return obs, sc, exq


@pytest.mark.parametrize("w", [1, 2, 3, 7, 8, 20, 64, 1024])
def test_hand_made_tables_with_a_ring_an_unplaced_contig_and_a_contig_of_one(w):
    from instagraal_amd import orientation_support as osup

    dist, stot, contig, placed, position, row, col, cnt = _hand_made()
    got = osup.support_host(dist, stot, contig, placed, position, row, col, cnt, HAND_FIRST, HAND_LAST, w, model_q=_toy_model_q)
    assert got["n_placed"] == 126 and got["n_seg"] == 12 and got["window"] == w
    geo = got["geometry"]
    assert geo.dtype == np.int32 and geo.shape == (12, 4) and got["observed"].dtype == np.int64 and got["expected_q"].shape == (12, 2)
    # every status; the geometry at both ends of the contig of 40 and of the contig of 60
    assert geo[:, 0].tolist() == [0, 0, 0, 0, 1, 0, 2, 1, 1, 0, 0, 0]
    n = HAND_LAST - HAND_FIRST + 1
    lin = np.array([0, 1, 2, 3, 4, 5, 8, 9, 10, 11])
    assert np.array_equal(geo[lin, 1], np.minimum(n[lin] // 2, w)) and not geo[[6, 7], 1:].any()
    c_start, c_end = np.where(HAND_FIRST < 40, 0, np.where(HAND_FIRST == 65, 65, 66)), np.where(HAND_FIRST < 40, 40, np.where(HAND_FIRST == 65, 66, 126))
    assert np.array_equal(geo[lin, 2], np.minimum(w, HAND_FIRST - c_start)[lin]) and np.array_equal(geo[lin, 3], np.minimum(w, c_end - 1 - HAND_LAST)[lin])
    assert geo[0, 2] == 0 and geo[0, 3] == min(w, 36) and geo[5, 3] == 0 and geo[5, 2] == min(w, 36) and geo[9, 2] == 0 and geo[11, 3] == 0
    # against the definition with loops
    obs, sc, exq = _brute(dist, stot, contig, placed, position, row, col, cnt, HAND_FIRST, HAND_LAST, geo, w, _toy_model_q)
    assert np.array_equal(got["observed"], obs) and np.array_equal(got["expected_q"], exq)
    assert all(got[k] == sc[k] for k in sc), (sc, {k: got[k] for k in sc})
    # the class identity and the bounds of the entries
    assert osup.observed_total(got) == int(cnt.sum()) and all(got[k] > 0 for k in osup.CLASS_SCALARS)
    assert got["counted"] <= got["entries_observed"] == int(obs.sum()) <= 2 * got["counted"] and got["n_judged"] == 8
    # rows that are not judged are zero; judged rows expect something in both classes
    idle = geo[:, 0] != 0
    assert not got["observed"][idle].any() and not got["expected_q"][idle].any() and (got["expected_q"][~idle] > 0).all()
    d = osup.derived(got)
    assert np.array_equal(d["pairs"], geo[:, 1].astype(np.int64) * (geo[:, 2] + geo[:, 3])) and np.array_equal(d["keep"], obs[:, 0] + obs[:, 3])
    # without a model: the same, less expected_q
    lean = osup.support_host(dist, stot, contig, placed, position, row, col, cnt, HAND_FIRST, HAND_LAST, w)
    assert lean["expected_q"] is None and np.array_equal(lean["observed"], obs) and "llr" not in osup.derived(lean)
    # no segment at all: every linear cis contact is uncounted
    none = osup.support_host(dist, stot, contig, placed, position, row, col, cnt, np.zeros(0, np.int64), np.zeros(0, np.int64), w, model_q=_toy_model_q)
    assert none["observed"].shape == (0, 4) and none["counted"] == none["within_segment"] == 0 and osup.observed_total(none) == int(cnt.sum())


def test_arguments_are_checked():
    from instagraal_amd import orientation_support as osup

    t = _hand_made()
    for bad in (0, 1025, 2.5):
        with pytest.raises(ValueError, match="window"):
            osup.support_host(*t, HAND_FIRST, HAND_LAST, bad)
    for first, last, what in (([5, 5], [6, 8], "ascending"), ([10, 2], [12, 4], "ascending"), ([38], [42], "two contigs"), ([0], [126], "range"),
                              ([-1], [3], "range"), ([4], [3], "range"), ([1, 2], [3], "one length"), ([1.0], [3.0], "integer")):
        with pytest.raises(ValueError, match=what):
            osup.support_host(*t, np.array(first), np.array(last), 8)
    assert osup.DEFAULT_WINDOW == 8 and osup.check_window(1024) == 1024


def _distance_contacts(rng, T, scale=6.0, n=60000):
    """contacts between TRUE positions, their number falling with the distance"""
    a = rng.randint(0, T, n)
    d = np.maximum(1, np.rint(rng.exponential(scale, n))).astype(np.int64)
    b = a + d
    ok = b < T
    return a[ok], b[ok], rng.randint(1, 5, int(ok.sum()))


def test_a_reversal_in_place_swaps_the_quadrants_exactly_and_ranks_first():
    from instagraal_amd import orientation_support as osup

    rng = np.random.RandomState(3)
    T = 300  # one linear contig; sub-fragment s sits at true position s
    dist = np.cumsum(rng.uniform(0.5, 2.5, T)).astype(np.float32)
    stot, contig, placed = np.zeros(T, np.float32), np.full(T, 4), np.ones(T, bool)
    a, b, cnt = _distance_contacts(rng, T)
    first, last = np.arange(0, T, 6), np.arange(0, T, 6) + 5  # 50 segments of 6 positions
    k_rev = 23
    f, l = int(first[k_rev]), int(last[k_rev])
    true_pos = np.arange(T)
    rev_pos = true_pos.copy()
    rev_pos[f:l + 1] = np.arange(l, f - 1, -1)  # the segment placed the wrong way round
    dist_rev = dist[rev_pos]  # (a sub-fragment's coordinate is that of the position it is placed at)
    for w in (1, 3, 4, 64):
        true = osup.support_host(dist, stot, contig, placed, true_pos, a, b, cnt, first, last, w, model_q=_toy_model_q)
        rev = osup.support_host(dist_rev, stot, contig, placed, rev_pos, a, b, cnt, first, last, w, model_q=_toy_model_q)
        assert np.array_equal(rev["observed"][k_rev], true["observed"][k_rev][[osup.RL, osup.RR, osup.LL, osup.LR]]), w
        assert np.array_equal(rev["geometry"], true["geometry"]) and osup.observed_total(rev) == osup.observed_total(true) == int(cnt.sum())
        assert rev["within_segment"] == true["within_segment"]
        others = np.setdiff1d(np.arange(first.size), [k_rev - 1, k_rev, k_rev + 1])  # (the neighbours see the reversed arms in their flanks)
        assert np.array_equal(rev["observed"][others], true["observed"][others])
        dt, dr = osup.derived(true), osup.derived(rev)
        assert dt["keep"][k_rev] > dt["flip"][k_rev] and dr["flip"][k_rev] == dt["keep"][k_rev] and dr["keep"][k_rev] == dt["flip"][k_rev]
        for res in (rev, dict(rev, expected_q=None)):  # by llr, and by z without the model
            top = osup.inverted_segments(res, 3)
            assert top.size >= 1 and top["segment"][0] == k_rev and top["flip"][0] > top["keep"][0], w
            assert (top["first"][0], top["last"][0], top["status"][0]) == (f, l, 0)
        assert osup.inverted_segments(rev, 5, min_observed=10 ** 9).size == 0
        if w >= 3:
            assert k_rev not in osup.inverted_segments(true, 50)["segment"]
    # the llr has the sign of flip - keep where the model expects more of the pairs that keep
    d = osup.derived(rev)
    ok = np.isfinite(d["llr"]) & (d["expected_keep"] > d["expected_flip"])
    assert ok.any() and np.array_equal(np.sign(d["llr"][ok]), np.sign(d["flip"][ok] - d["keep"][ok]))
    assert np.isinf(osup.derived(dict(geometry=np.zeros((1, 4), np.int32), observed=np.array([[0, 1, 0, 0]]), expected_q=None))["ratio"][0])
    assert np.isnan(osup.derived(dict(geometry=np.zeros((1, 4), np.int32), observed=np.zeros((1, 4), np.int64), expected_q=None))["ratio"][0])


def _state_tables(prob):
    S = prob.S_o_A_frags
    return dict(id_c=S["id_c"].astype(np.int64), pos=S["pos"].astype(np.int64), ori=np.ones(prob.n_frags, np.int64), id_d=S["id_d"].astype(np.int64))


def _order_of(id_c, pos, ori, sub_first, sub_len):
    """the genome order of a state of placed contigs: contigs by id, bins by pos, the sub-fragments of a bin by its orientation"""
    order = []
    for b in np.lexsort((pos, id_c)).tolist():
        subs = np.arange(sub_first[b], sub_first[b] + sub_len[b])
        order.append(subs if ori[b] == 1 else subs[::-1])
    return np.concatenate(order)


def test_bin_segments_and_block_segments_on_the_three_state_situations():
    from instagraal_amd import orientation_support as osup, synth

    prob = synth.make_problem(*synth.CONFIGS["small"])
    st = _state_tables(prob)
    parent = prob.np_sub_frags_2_frags["x"].astype(np.int64)
    N, M = prob.n_frags, parent.size
    sub_len = np.bincount(parent, minlength=N)
    sub_first = np.cumsum(sub_len) - sub_len
    init_c, init_p = st["id_c"].copy(), st["pos"].copy()
    # fresh: the order is the table's; one bin segment per bin, one block per contig, every block without a flank
    order = _order_of(st["id_c"], st["pos"], st["ori"], sub_first, sub_len)
    assert np.array_equal(order, np.arange(M))
    b = osup.bin_segments(order, parent)
    assert np.array_equal(b["first_bin"], np.arange(N)) and np.array_equal(b["last_bin"], b["first_bin"])
    assert np.array_equal(b["first"], sub_first) and np.array_equal(b["last"], sub_first + sub_len - 1)
    blocks = osup.block_segments(order, parent, st["id_c"], st["ori"], st["id_d"], init_c, init_p)
    n_contigs = np.unique(st["id_c"]).size
    assert blocks["first"].size == n_contigs and np.array_equal(st["pos"][blocks["first_bin"]], np.zeros(n_contigs, np.int64))
    assert np.array_equal(blocks["last"][:-1] + 1, blocks["first"][1:]) and blocks["first"][0] == 0 and blocks["last"][-1] == M - 1
    contig = st["id_c"][parent]
    res = osup.support_host(np.arange(M, dtype=np.float32), np.zeros(M, np.float32), contig, np.ones(M, bool), np.arange(M), prob.coo_row, prob.coo_col,
                            prob.coo_cnt, blocks["first"], blocks["last"], 8)
    assert set(res["geometry"][:, 0].tolist()) <= {osup.STATUS_NO_FLANK, osup.STATUS_SHORT} and (res["geometry"][:, 0] == osup.STATUS_NO_FLANK).sum() >= n_contigs - 5
    assert res["n_judged"] == 0 and not res["observed"].any() and res["counted"] == 0
    # behind the bomb: every bin a contig of its own -> one block per bin
    bomb_c = np.arange(N, dtype=np.int64) + 1
    blocks = osup.block_segments(order, parent, bomb_c, st["ori"], st["id_d"], init_c, init_p)
    assert np.array_equal(blocks["first"], b["first"]) and np.array_equal(blocks["last"], b["last"]) and np.array_equal(blocks["first_bin"], np.arange(N))
    # hand-edited: bins 10 .. 14 of the first long contig reversed as a run (their order and their orientations), bin 20 flipped alone
    c0 = int(np.bincount(st["id_c"]).argmax())  # the longest contig
    bins = np.nonzero(st["id_c"] == c0)[0]
    assert bins.size >= 24
    pos, ori = st["pos"].copy(), st["ori"].copy()
    run = bins[10:15]
    pos[run] = pos[run][::-1]
    ori[run] = -1
    ori[bins[20]] = -1
    order = _order_of(st["id_c"], pos, ori, sub_first, sub_len)
    blocks = osup.block_segments(order, parent, st["id_c"], ori, st["id_d"], init_c, init_p)
    inside = np.nonzero(st["id_c"][blocks["first_bin"]] == c0)[0]
    assert [(int(blocks["first_bin"][k]), int(blocks["last_bin"][k])) for k in inside] == [
        (bins[0], bins[9]), (bins[14], bins[10]), (bins[15], bins[19]), (bins[20], bins[20]), (bins[21], bins[-1])]
    assert blocks["first"].size == n_contigs + 4
    k = inside[1]
    assert blocks["last"][k] - blocks["first"][k] + 1 == sub_len[run].sum()
    # a run that is reversed in the order but not in its orientations is no block: its bins stand alone
    ori2 = st["ori"].copy()
    blocks2 = osup.block_segments(_order_of(st["id_c"], pos, ori2, sub_first, sub_len), parent, st["id_c"], ori2, st["id_d"], init_c, init_p)
    assert blocks2["first"].size == n_contigs + 6
    # nothing placed
    empty = osup.block_segments(np.zeros(0, np.int64), parent, st["id_c"], ori, st["id_d"], init_c, init_p)
    assert all(empty[k].size == 0 for k in ("first", "last", "first_bin", "last_bin"))


@pytest.mark.parametrize("name", FIXTURES)
def test_keep_plus_flip_is_the_reference_matrix_summed_over_the_arm_flank_rectangles(name, oracle_lib):
    from instagraal_amd import orientation_support as osup, synth
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
    assert T == prob.n_sub_frags and not stot.any()
    position = np.empty(T, np.int64)
    position[order] = np.arange(T)
    parent = prob.np_sub_frags_2_frags["x"].astype(np.int64)
    col = {k: state[i].astype(np.int64) for i, k in enumerate(oracle_lib.FRAG_FIELDS)}
    S0 = prob.S_o_A_frags
    lists = [osup.bin_segments(order, parent), osup.block_segments(order, parent, col["id_c"], col["ori"], col["id_d"], S0["id_c"], S0["pos"])]
    judged_somewhere = 0
    for seg in lists:
        first, last = seg["first"], seg["last"]
        assert np.array_equal(seg["first_bin"], parent[order[first]]) and np.array_equal(seg["last_bin"], parent[order[last]])
        for w in (1, 2, 8, 64):
            got = osup.support_host(dist, stot, contig, np.ones(T, bool), position, prob.coo_row, prob.coo_col, prob.coo_cnt, first, last, w)
            assert osup.observed_total(got) == int(prob.coo_cnt.astype(np.int64).sum())
            d = osup.derived(got)
            for k in range(first.size):
                status, m, lf, rf = (int(x) for x in got["geometry"][k])
                f, l = int(first[k]), int(last[k])
                arms = np.r_[f:f + m, l - m + 1:l + 1]
                flanks = np.r_[f - lf:f, l + 1:l + 1 + rf]
                want = int(matrix[np.ix_(arms, flanks)].sum()) if status == 0 else 0
                assert int(d["keep"][k] + d["flip"][k]) == want, (name, w, k)
                if status == 0:  # the quadrants one by one
                    la, ra, lfl, rfl = np.r_[f:f + m], np.r_[l - m + 1:l + 1], np.r_[f - lf:f], np.r_[l + 1:l + 1 + rf]
                    assert got["observed"][k].tolist() == [int(matrix[np.ix_(x, y)].sum()) for x, y in ((la, lfl), (la, rfl), (ra, lfl), (ra, rfl))]
            judged_somewhere += got["n_judged"]
    assert judged_somewhere > 0 or name.endswith("bomb")


def test_write_orientations(tmp_path):
    from instagraal_amd import orientation_support as osup

    t = _hand_made()
    res = osup.support_host(*t, HAND_FIRST, HAND_LAST, 8, model_q=_toy_model_q)
    path = str(tmp_path / "orientations.txt")
    osup.write_orientations(path, res)
    lines = open(path).read().splitlines()
    assert lines[0][2:].split() == list(osup.COLUMNS)
    rows = [ln.split() for ln in lines if not ln.startswith("#")]
    assert len(rows) == res["n_judged"] == 8 and all(len(r) == len(osup.COLUMNS) for r in rows)
    d = osup.derived(res)
    for r in rows:
        k = int(r[0])
        assert [int(x) for x in r[10:14]] == res["observed"][k].tolist() and int(r[14]) == d["keep"][k] and int(r[15]) == d["flip"][k]
        assert (int(r[1]), int(r[2])) == (HAND_FIRST[k], HAND_LAST[k]) and int(r[6]) == 0
    sc = dict(kv.split("=") for kv in lines[-1][2:].split())
    assert int(sc["window"]) == 8 and sum(int(sc[k]) for k in osup.CLASS_SCALARS) == int(t[7].sum()) and int(sc["n_judged"]) == 8
    osup.write_orientations(path, res, mode="a", title="again")
    assert open(path).read().count("# again") == 1 and len(open(path).read().splitlines()) == 2 * len(lines) + 1


def test_import_needs_neither_matplotlib_nor_the_library():
    code = ("import sys; sys.modules['matplotlib'] = None; sys.modules['ctypes'] = None\n"
            "from instagraal_amd import orientation_support as o; print(o.DEFAULT_WINDOW, len(o.SCALARS))")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.split() == ["8", "8"], out.stderr
