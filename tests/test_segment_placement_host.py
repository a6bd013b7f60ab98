"""CPU tests of the segment placement's rule (instagraal_amd.segment_placement): ``support_host`` against an independent dense brute
force on ``tiny`` -- the symmetric matrix permuted by the genome order, the guest's rows and columns deleted, the window rectangles
summed, the quadrants by arm masks --, ``support_sparse`` (the device's route) against the enumeration, every identity of the module's
docstring, the planted block the feature exists for, the ranking and the file, the arguments, and that the states the GPU tests use
exercise what they are there for.  Every comparison is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_placement_support_host import _contacts, _exact_best, _genome, _lay_out, _masks, _problem

WINDOWS = (1, 2, 4, 64, 1024)
STATES = dict(fresh={}, permuted=dict(seed=5), ring=dict(seed=6, ring=True), single=dict(seed=7, single=True), unplaced=dict(seed=8, unplaced=True),
              bombed=dict(bombed=True))


def _tables(prob, genome):
    stot, contig, placed, position, parent, _ = _lay_out(prob, genome)
    return stot, contig, placed, position


def _order(placed, position):
    order = np.nonzero(placed)[0]
    return order[np.argsort(position[order])]


def _per_position(stot, contig, placed, position):
    """-> order, contig_start, contig_end, ring: per position"""
    from instagraal_amd.junction_profile import contig_runs

    members, start, length = contig_runs(contig, position)
    return members, np.repeat(start, length), np.repeat(start + length, length), np.asarray(stot)[members] != 0


def _groups(seg, c_start, size, every=1):
    """runs of ``size`` neighbouring bin segments of one contig as segments (a shorter run at a contig's tail stays), every ``every``-th"""
    first, last = [], []
    i, n = 0, seg["first"].size
    while i < n:
        j = i
        while j + 1 < n and j + 1 < i + size and c_start[seg["first"][j + 1]] == c_start[seg["first"][i]]:
            j += 1
        first.append(seg["first"][i])
        last.append(seg["last"][j])
        i = j + 1
    return np.asarray(first[::every], np.int64), np.asarray(last[::every], np.int64)


def _lists(prob, t):
    """the segment lists the tests run over: name -> (first, last)"""
    from instagraal_amd import segment_placement as sp

    parent = prob.np_sub_frags_2_frags["x"].astype(np.int64)
    order, cs, ce, ring = _per_position(*t)
    b = sp.bin_segments(order, parent)
    sc = sp.scaffold_segments(order, cs, ce, ring)
    none = np.zeros(0, np.int64)
    return dict(bins=(b["first"], b["last"]), pairs=_groups(b, cs, 2), triples=_groups(b, cs, 3), gappy=_groups(b, cs, 2, every=3),
                scaffolds=(sc["first"], sc["last"]), empty=(none, none))


def _brute(t, contacts, first, last, w, min_hosts_list):
    """the definition on the dense matrix -> {min_hosts: {name: values}}, and the scalars"""
    from instagraal_amd import segment_placement as sp

    stot, contig, placed, position = t
    row, col, cnt = contacts
    M = position.size
    D = np.zeros((M, M), np.int64)
    np.add.at(D, (row, col), cnt)
    D = D + D.T
    order = _order(placed, position)
    T = order.size
    Dp = D[order][:, order]
    label = np.where(stot[order] != 0, -1, contig[order])
    Dp[label < 0, :] = 0
    Dp[:, label < 0] = 0
    runs = []  # the linear contigs in the order of their positions
    for p in range(T):
        if label[p] >= 0 and (p == 0 or contig[order[p]] != contig[order[p - 1]]):
            runs.append(int(label[p]))
    n_seg = len(first)
    out = {}
    for mh in min_hosts_list:
        o = {k: np.zeros(n_seg, np.int32 if k in sp.INT_ARRAYS else np.int64) for k in sp.ARRAYS}
        for k in sp.CONTIG_FIELDS:
            o[k][:] = -1
        o["quadrants"] = np.zeros((n_seg, 3, 4), np.int64)
        out[mh] = o
    everything = np.arange(T)
    for i in range(n_seg):
        mine = np.arange(first[i], last[i] + 1)
        if label[mine[0]] < 0:
            for mh in min_hosts_list:
                out[mh]["status"][i] = 2
            continue
        k_own = int(label[mine[0]])
        m = min(mine.size // 2, w)
        rows_of = dict(H=Dp[mine[:m]].sum(axis=0) if m else np.zeros(T, np.int64), T=Dp[mine[mine.size - m:]].sum(axis=0) if m else np.zeros(T, np.int64),
                       all=Dp[mine].sum(axis=0))
        red = {k: np.delete(v, mine) for k, v in rows_of.items()}
        lab = np.delete(label, mine)
        sk, su, sums, hosts = [], [], [], []
        home = None
        for ki, kk in enumerate(runs):
            where = np.nonzero(lab == kk)[0]
            n = where.size
            if kk == k_own:
                uh = int(mine[0] - np.nonzero(label == kk)[0][0])
                if n == 0:
                    continue
            L, R = _masks(n, w)
            per = [(L @ red[key][where], R @ red[key][where]) for key in ("all", "H", "T")]
            u = np.arange(n + 1)
            if kk == k_own:
                home = len(np.concatenate(sk)) + uh if sk else uh
            sk.append(np.full(n + 1, ki))
            su.append(u)
            sums.append(np.stack([per[0][0], per[0][1], per[1][0], per[1][1], per[2][0], per[2][1]], axis=1))
            hosts.append(np.minimum(n, u + w) - np.maximum(0, u - w))
        ki_own = runs.index(k_own)
        uh = int(mine[0] - np.nonzero(label == k_own)[0][0])
        sk, su = (np.concatenate(a) if a else np.zeros(0, np.int64) for a in (sk, su))
        sums = np.concatenate(sums) if sums else np.zeros((0, 6), np.int64)
        hosts = np.concatenate(hosts) if hosts else np.zeros(0, np.int64)
        obs = sums[:, 0] + sums[:, 1]
        for mh in min_hosts_list:
            o = out[mh]
            o["contig"][i], o["offset"][i], o["n_positions"][i], o["arm"][i] = ki_own, uh, mine.size, m
            picks = [home]
            ok = (hosts >= mh) & ~((sk == ki_own) & (np.abs(su - uh) < 2 * w))
            b = _exact_best(obs, hosts, ok)
            picks.append(b if b >= 0 else None)
            s = _exact_best(obs, hosts, ok & ~((sk == sk[b]) & (np.abs(su - su[b]) < 2 * w))) if b >= 0 else -1
            picks.append(s if s >= 0 else None)
            for site, (name, j) in enumerate(zip(("home", "best", "second"), picks)):
                if j is None:
                    continue
                if name != "home":
                    o[name + "_contig"][i], o[name + "_offset"][i] = sk[j], su[j]
                o[name + "_hosts"][i], o[name + "_left"][i], o[name + "_right"][i] = hosts[j], sums[j, 0], sums[j, 1]
                o["quadrants"][i, site] = sums[j, 2:]
    # the scalars, contact by contact
    seg = np.full(T, -1, np.int64)
    for i in range(n_seg):
        seg[first[i]:last[i] + 1] = i
    sc = dict.fromkeys(sp.SCALARS, 0)
    n_counted = 0
    ring_sub = stot != 0
    for r, c, v in zip(row.tolist(), col.tolist(), cnt.tolist()):
        if not (placed[r] and placed[c]):
            sc["unplaced_observed"] += v
        elif ring_sub[r] or ring_sub[c]:
            sc["ring_observed"] += v
        else:
            a, b = seg[position[r]], seg[position[c]]
            if a >= 0 and a == b:
                sc["within_segment_observed"] += v
            elif a < 0 and b < 0:
                sc["uncounted_observed"] += v
            else:
                sc["counted_observed"] += v
                sc["entries"] += int(a >= 0) + int(b >= 0)
                n_counted += 1
    sc.update(n_contigs=len(runs), n_placed=T, n_guests=int(sum(label[f] >= 0 for f in first)))
    return out, sc, n_counted


def _assert_equal(got, want, what, scalars=None):
    from instagraal_amd import segment_placement as sp

    for k in sp.ARRAYS + ("quadrants",):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k, np.argwhere(got[k] != want[k])[:5].tolist())
    for k in sp.SCALARS:
        if scalars is not None or k in want:
            assert got[k] == (scalars or want)[k], (what, k, got[k], (scalars or want)[k])


def _min_hosts(w):
    return sorted({1, w, 2 * w})


@pytest.mark.parametrize("state", sorted(STATES))
def test_support_host_and_sparse_equal_the_dense_brute_force(state):
    from instagraal_amd import segment_placement as sp

    prob = _problem("tiny")
    t = _tables(prob, _genome(prob, **STATES[state]))
    contacts = _contacts(prob)
    total = int(contacts[2].sum())
    lists = _lists(prob, t)
    full = state in ("fresh", "permuted")
    for name, (first, last) in lists.items():
        for w in WINDOWS if full or name in ("pairs", "scaffolds") else (4,):
            if state == "bombed" and (w > 4 or name not in ("bins", "scaffolds", "empty")):
                continue
            brute, sc, n_counted = _brute(t, contacts, first, last, w, _min_hosts(w))
            for mh in _min_hosts(w):
                host = sp.support_host(*t, *contacts, first, last, w, mh)
                _assert_equal(host, brute[mh], (state, name, w, mh, "host"), scalars=sc)
                sparse = sp.support_sparse(*t, *contacts, first, last, w, mh)
                _assert_equal(sparse, host, (state, name, w, mh, "sparse"))
                # the identities
                assert sp.observed_total(host) == total and n_counted == host["n_counted_contacts"] <= host["entries"] <= 2 * n_counted
                q = host["quadrants"]
                for s, which in enumerate(sp.SITES):
                    left, right = host[which + "_left"], host[which + "_right"]
                    assert np.all(q[:, s, sp.HL] + q[:, s, sp.TL] <= left) and np.all(q[:, s, sp.HR] + q[:, s, sp.TR] <= right)
                    whole = host["n_positions"] == 2 * host["arm"]
                    assert np.array_equal((q[:, s, sp.HL] + q[:, s, sp.TL])[whole], left[whole]) and np.array_equal((q[:, s, sp.HR] + q[:, s, sp.TR])[whole], right[whole])
                assert int(host["rowptr"][-1]) <= host["entries"] == int(host["row_entries"].sum()) and int(host["count"].sum()) <= 2 * host["counted_observed"]
    if state == "ring":
        assert any((sp.support_host(*t, *contacts, f, l, 4)["status"] == 2).any() for f, l in lists.values())
    if state in ("single", "bombed"):  # a contig that is one segment: no home
        r = sp.support_host(*t, *contacts, *lists["scaffolds"], 4, 1)
        assert np.all(r["home_hosts"] == 0) and (r["best_contig"] >= 0).any()


@pytest.mark.parametrize("state", ["fresh", "permuted", "ring", "single", "unplaced"])
def test_bin_segments_of_the_whole_order_equal_the_bin_level_report(state):
    from instagraal_amd import placement_support as ps, segment_placement as sp

    prob = _problem("tiny")
    lay = _lay_out(prob, _genome(prob, **STATES[state]))
    t, contacts = lay[:4], _contacts(prob)
    order = _order(t[2], t[3])
    seg = sp.bin_segments(order, lay[4])
    for w in (1, 4, 8, 64):
        for mh in (1, w):
            a = sp.support_host(*t, *contacts, seg["first"], seg["last"], w, mh)
            b = ps.support_host(*lay, *contacts, w, mh)
            for k in ps.ARRAYS:
                assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k][seg["first_bin"]]), (state, w, mh, k)
            assert a["uncounted_observed"] == 0 and a["within_segment_observed"] == b["within_bin_observed"] and a["entries"] == b["entries"]
            assert all(a[k] == b[k] for k in ("unplaced_observed", "ring_observed", "counted_observed", "n_contigs"))


@pytest.mark.parametrize("state", ["fresh", "permuted", "ring", "single"])
def test_home_quadrants_equal_the_orientation_support(state):
    from instagraal_amd import orientation_support as osup, segment_placement as sp

    prob = _problem("tiny")
    t = _tables(prob, _genome(prob, **STATES[state]))
    contacts = _contacts(prob)
    dist = np.zeros(t[0].size, np.float32)
    for name, (first, last) in _lists(prob, t).items():
        for w in (1, 4, 8, 64):
            a = sp.support_host(*t, *contacts, first, last, w, 1)
            o = osup.support_host(dist, *t, *contacts, first, last, w)
            assert np.array_equal(a["quadrants"][:, 0, :], o["observed"]), (state, name, w)  # (HL, HR, TL, TR) == (LL, LR, RL, RR)
            assert np.array_equal(a["arm"][a["status"] == 0], o["geometry"][a["status"] == 0, 1])


def test_reversing_a_guest_in_place_swaps_the_quadrants_and_nothing_else():
    from instagraal_amd import segment_placement as sp

    prob = _problem("tiny")
    t = _tables(prob, _genome(prob, seed=5))
    contacts = _contacts(prob)
    first, last = _lists(prob, t)["triples"]
    swaps = 0
    for g in (1, first.size // 2, first.size - 2):
        f, l = int(first[g]), int(last[g])
        position = t[3].copy()
        inside = (position >= f) & (position <= l)
        position[inside] = f + l - position[inside]
        for w in (1, 4, 64):
            for fs, ls, at in ((first[g:g + 1], last[g:g + 1], 0), (first, last, g)):
                a = sp.support_host(*t, *contacts, fs, ls, w)
                b = sp.support_host(t[0], t[1], t[2], position, *contacts, fs, ls, w)
                for k in sp.ARRAYS:
                    assert a[k][at] == b[k][at], (g, w, k)
                assert all(a[k] == b[k] for k in sp.SCALARS)
                assert np.array_equal(a["quadrants"][at][:, [sp.TL, sp.TR, sp.HL, sp.HR]], b["quadrants"][at]), (g, w)
                swaps += int(a["quadrants"][at].any())
                if fs.size == 1:  # the guest alone: nothing else changes at all
                    _assert_equal(dict(b, quadrants=b["quadrants"][:, :, [sp.TL, sp.TR, sp.HL, sp.HR]]), a, ("alone", g, w))
    assert swaps > 6


def _flat(genome):
    return [dict(bins=list(c["bins"]), ring=c["ring"], placed=c["placed"], flips=set(c["bins"]) if c.get("flip") else set()) for c in genome]


def _lay_out_bins(prob, genome):
    """``_lay_out`` with the flip per bin (``flips``: the bins of a contig whose sub-fragments run backwards)"""
    parent = prob.np_sub_frags_2_frags["x"].astype(np.int64)
    M = parent.size
    stot, contig, placed, position = np.zeros(M, np.float32), np.zeros(M, np.int64), np.ones(M, bool), np.full(M, -1, np.int64)
    at = 0
    for k, c in enumerate(genome):
        for b in c["bins"]:
            s = np.nonzero(parent == b)[0]
            s = s[::-1] if b in c["flips"] else s
            contig[s] = k
            position[s] = at + np.arange(s.size)
            at += s.size
    return stot, contig, placed, position, parent, prob.n_frags


def _plant(prob, k, reverse=False):
    """the middle k bins of the longest contig moved, as they are (``reverse``: turned round), to the tail of the second longest ->
    (the layout, the block's bins, the contig it came from, the former offset in positions)"""
    g = _flat(_genome(prob))
    by_len = sorted(range(len(g)), key=lambda i: -len(g[i]["bins"]))
    src, dst = g[by_len[0]], g[by_len[1]]
    a = (len(src["bins"]) - k) // 2
    block = src["bins"][a:a + k]
    parent = prob.np_sub_frags_2_frags["x"].astype(np.int64)
    former = int(sum((parent == b).sum() for b in src["bins"][:a]))
    del src["bins"][a:a + k]
    dst["bins"] += block[::-1] if reverse else block
    if reverse:
        dst["flips"] |= set(block)
    return _lay_out_bins(prob, g), block, by_len[0], former


@pytest.mark.parametrize("cfg,w,k", [("tiny", 4, 3), ("small", 8, 4), ("small", 32, 4)])
def test_the_planted_block_is_found_as_a_segment_and_not_bin_by_bin(cfg, w, k):
    from instagraal_amd import placement_support as ps, segment_placement as sp

    prob = _problem(cfg)
    contacts = _contacts(prob)
    for reverse in (False, True):
        lay, block, src, former = _plant(prob, k, reverse)
        t, parent = lay[:4], lay[4]
        order = _order(t[2], t[3])
        b = sp.bin_segments(order, parent)
        mine = np.isin(b["first_bin"], block)
        i0 = int(np.nonzero(mine)[0][0])
        assert np.nonzero(mine)[0].tolist() == list(range(i0, i0 + k))  # the block lies in one piece
        first = np.concatenate([b["first"][:i0 + 1], b["first"][i0 + k:]])
        last = np.concatenate([b["last"][:i0], b["last"][i0 + k - 1:]])
        first_bin = np.concatenate([b["first_bin"][:i0 + 1], b["first_bin"][i0 + k:]])
        res = sp.support_host(*t, *contacts, first, last, w)
        res.update(sp.densities(res))
        res.update(sp.orientation_at(res))
        res.update(sp.sites_for_people(res, order, parent, np.zeros(prob.n_frags, np.int64)))
        print(cfg, w, k, reverse, "ratio", res["ratio"][i0], "second_ratio", res["second_ratio"][i0], "best", res["best_contig"][i0], res["best_offset"][i0], "former",
              former, "keep/flip", res["keep"][i0, 1], res["flip"][i0, 1])
        assert res["ratio"][i0] >= 10
        assert res["best_contig"][i0] == src and abs(int(res["best_offset"][i0]) - former) <= w
        assert res["second_ratio"][i0] < 0.5
        if reverse:
            assert res["flip"][i0, 1] > res["keep"][i0, 1] and res["verdict"][i0, 1] == "reversed"
        else:
            assert res["keep"][i0, 1] > res["flip"][i0, 1] and res["verdict"][i0, 1] == "as_placed"
        assert sp.misplaced_segments(res)["segment"][0] == i0 and sp.misplaced_segments(res)["first_bin"][0] == first_bin[i0] == block[-1 if reverse else 0]
        # the sentence the feature exists for: bin by bin the interior of the block is at home
        bins = ps.support_host(*lay, *contacts, w)
        ratio = ps.densities(bins)["ratio"]
        print("bin-level ratios of the block", ratio[block])
        assert np.all(ratio[block[1:-1]] < 1)


def _fake_result():
    from instagraal_amd import segment_placement as sp

    n = 6
    res = {k: np.zeros(n, np.int32 if k in sp.INT_ARRAYS else np.int64) for k in sp.ARRAYS}
    res.update(window=4, min_hosts=4, n_seg=n, first=np.arange(0, 60, 10), last=np.arange(9, 69, 10), status=np.array([0, 0, 0, 2, 0, 0], np.int32))
    res.update(contig=np.array([0, 0, 0, -1, 1, 1], np.int32), n_positions=np.where(res["status"] == 0, 10, 0).astype(np.int32),
               offset=np.array([0, 10, 20, 0, 0, 10], np.int32), arm=np.where(res["status"] == 0, 4, 0).astype(np.int32))
    res.update(home_hosts=np.full(n, 8, np.int32), home_left=np.array([10, 0, 5, 0, 5, 8]), home_right=np.array([10, 0, 5, 0, 5, 8]))
    res.update(best_contig=np.array([1, 1, 1, -1, 0, -1], np.int32), best_offset=np.array([3, 4, 5, 0, 6, 0], np.int32), best_hosts=np.array([8, 8, 4, 0, 8, 0], np.int32),
               best_left=np.array([5, 3, 10, 0, 10, 0]), best_right=np.array([5, 3, 0, 0, 10, 0]))
    for k in ("second_contig",):
        res[k][:] = -1
    q = np.zeros((n, 3, 4), np.int64)
    q[0, 1] = (3, 1, 1, 3)
    q[1, 1] = (1, 2, 2, 1)
    q[2, 1] = (2, 2, 2, 2)
    res["quadrants"] = q
    res.update(dict.fromkeys(sp.SCALARS, 7))
    res.update(first_position=np.array([0, 40], np.int32), contig_positions=np.array([30, 20], np.int32))
    return res


def test_the_ranking_the_verdicts_and_the_file(tmp_path):
    from instagraal_amd import segment_placement as sp

    res = _fake_result()
    order = np.arange(60)
    parent = order // 5
    res.update(sp.densities(res))
    at = sp.orientation_at(res)
    assert at["keep"][:3, 1].tolist() == [6, 2, 4] and at["flip"][:3, 1].tolist() == [2, 4, 4]
    assert at["verdict"][:3, 1].tolist() == ["as_placed", "reversed", "undecided"] and at["verdict"][3, 1] == "undecided"
    res.update(at)
    res.update(sp.sites_for_people(res, order, parent, np.arange(12) // 6 + 3))
    assert res["first_bin"].tolist() == [0, 2, 4, 6, 8, 10] and res["last_bin"].tolist() == [1, 3, 5, 7, 9, 11]
    assert res["scaffold"].tolist() == [3, 3, 3, -1, 4, 4]
    assert np.isinf(res["ratio"][1]) and res["ratio"][0] == 0.5 and res["ratio"][2] == 2.0 and res["ratio"][4] == 2.0 and res["ratio"][5] == 0.0 and np.isnan(res["ratio"][3])
    ranked = sp.misplaced_segments(res)
    assert ranked["segment"].tolist() == [1, 2, 4]  # inf first, ties by segment index
    assert sp.misplaced_segments(res, n=1)["segment"].tolist() == [1] and sp.misplaced_segments(res, min_ratio=0.0)["segment"].tolist() == [1, 2, 4, 0]
    assert ranked.dtype == sp.SEGMENT_DTYPE and ranked["best_scaffold"].tolist() == [4, 4, 3]
    path = str(tmp_path / "segment_placements.txt")
    assert sp.write_segment_placements(path, res, title="level=block") == 3
    assert sp.write_segment_placements(path, res, n=1, mode="a", title="level=scaffold") == 1
    lines = open(path).read().splitlines()
    assert lines[0] == "# level=block" and lines[1][2:].split() == list(sp.FILE_COLUMNS) and lines[6] == "# level=scaffold"
    rows = [ln.split() for ln in lines if not ln.startswith("#")]
    assert [int(r[0]) for r in rows] == [1, 2, 4, 1] and rows[0][-3:] == ["2", "4", "reversed"] and rows[1][-1] == "undecided"
    assert all(len(r) == len(sp.FILE_COLUMNS) for r in rows)
    tail = dict(kv.split("=") for kv in lines[5][2:].split())
    assert tail["window"] == "4" and tail["min_hosts"] == "4" and all(tail[k] == "7" for k in sp.SCALARS)


def test_arguments_and_the_overflow_guard():
    from instagraal_amd import segment_placement as sp

    prob = _problem("tiny")
    t = _tables(prob, _genome(prob))
    contacts = _contacts(prob)
    first, last = _lists(prob, t)["pairs"]
    for bad in (0, 1025, 2.5):
        with pytest.raises(ValueError, match="window"):
            sp.support_host(*t, *contacts, first, last, bad)
    for w, bad in ((4, 0), (4, 9), (1, 3), (8, 1.5)):
        with pytest.raises(ValueError, match="segment placement.*min_hosts"):
            sp.support_host(*t, *contacts, first, last, w, bad)
    T = int((t[3] >= 0).sum())
    for f, l, what in ((first[::-1], last[::-1], "not ascending and disjoint"), (np.array([0, 3]), np.array([3, 5]), "not ascending and disjoint"),
                       (np.array([-1]), np.array([2]), "out of range"), (np.array([5]), np.array([T]), "out of range"), (np.array([5]), np.array([4]), "out of range"),
                       (np.array([0]), np.array([T - 1]), "spans two contigs"), (np.array([0.5]), np.array([2.0]), "integer vectors"),
                       (np.array([0, 1]), np.array([2]), "integer vectors")):
        for rule in (sp.support_host, sp.support_sparse):
            with pytest.raises(ValueError, match="segment placement: segment list.*" + what):
                rule(*t, *contacts, f, l, 4)
    with pytest.raises(ValueError, match="placed and position disagree"):
        sp.support_host(t[0], t[1], ~t[2], t[3], *contacts, first, last, 4)
    row, col, cnt = contacts
    big = np.array([1 << 51], np.int64)
    with pytest.raises(ValueError, match="segment placement: counts too large for this window"):
        sp.support_host(*t, row[:1], col[:1], big, first, last, 1024)
    assert sp.observed_total(sp.support_host(*t, row[:1], col[:1], big - 1, first, last, 1024)) == (1 << 51) - 1
    with pytest.raises(ValueError, match="counts too large"):
        sp.support_sparse(*t, row[:2], col[:2], np.array([1 << 60, 1 << 60]), first, last, 1)
    assert sp.SCALARS == ("unplaced_observed", "ring_observed", "within_segment_observed", "counted_observed", "uncounted_observed", "entries", "n_contigs",
                          "n_guests", "n_placed")
    assert sp.INT_ARRAYS[-1] == "arm" and sp.INT_ARRAYS[:-1] == sp.ps.INT_ARRAYS and sp.LONG_ARRAYS == sp.ps.LONG_ARRAYS


def test_nothing_placed_and_no_contacts():
    from instagraal_amd import segment_placement as sp

    prob = _problem("tiny")
    none = np.zeros(0, np.int64)
    t = _tables(prob, _genome(prob, nothing=True))
    r = sp.support_host(*t, *_contacts(prob), none, none, 4)
    assert r["n_placed"] == 0 == r["n_contigs"] == r["entries"] and r["unplaced_observed"] == int(prob.coo_cnt.astype(np.int64).sum()) and r["quadrants"].shape == (0, 3, 4)
    with pytest.raises(ValueError, match="out of range"):
        sp.support_host(*t, *_contacts(prob), np.array([0]), np.array([0]), 4)
    t = _tables(prob, _genome(prob))
    first, last = _lists(prob, t)["pairs"]
    for rule in (sp.support_host, sp.support_sparse):
        r = rule(*t, none, none, none, first, last, 4)
        assert r["n_guests"] == first.size and not (r["best_contig"] >= 0).any() and (r["home_hosts"] > 0).all() and not r["quadrants"].any()


def test_the_states_of_the_gpu_tests_have_segment_rows_on_both_sides_of_the_scan_threshold():
    from instagraal_amd import segment_placement as sp

    prob = _problem("small")
    lay = _lay_out(prob, _genome(prob))
    t = lay[:4]
    order = _order(t[2], t[3])
    b = sp.bin_segments(order, lay[4])
    _, cs, ce, ring = _per_position(*t)
    sc = sp.scaffold_segments(order, cs, ce, ring)
    for first, last in ((b["first"], b["last"]), _groups(b, cs, 4), (sc["first"], sc["last"])):
        r = sp.support_sparse(*t, *_contacts(prob), first, last, 64, 1)
        n = np.diff(r["rowptr"])[r["status"] == 0]
        assert (n <= sp.WAVE_ENTRIES).any() or first.size == sc["first"].size
        assert (n > sp.WAVE_ENTRIES).any()
    assert sp.WAVE_ENTRIES == 128


def test_the_module_imports_without_the_library():
    code = ("import sys; import instagraal_amd.segment_placement as sp; "
            "assert 'instagraal_amd.hip_lib' not in sys.modules and 'torch' not in sys.modules, sorted(m for m in sys.modules if 'hip' in m or m == 'torch'); "
            "print(len(sp.SCALARS))")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0 and r.stdout.strip() == "9", r.stderr[-2000:]
