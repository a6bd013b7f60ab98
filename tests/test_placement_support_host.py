"""CPU tests of the placement support's rule (instagraal_amd.placement_support): ``support_host`` against an independent dense brute
force on ``tiny`` -- the symmetric matrix permuted by the genome order, the guest's rows and columns deleted, the window rectangles
summed --, ``candidate_sites`` (what the device visits) against the enumeration of every site, the identities, the tie rule, the
ranking and the file, the planted misplacement, and that the states the GPU tests use exercise what they are there for.  Every
comparison is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

WINDOWS = (1, 2, 4, 64, 1024)


def _problem(cfg="tiny"):
    from instagraal_amd import synth

    return synth.make_problem(*synth.CONFIGS[cfg])


def _contigs_of(prob):
    """the problem's contigs as lists of bins in the table's order"""
    S = prob.S_o_A_frags
    out = []
    for c in np.unique(S["id_c"]).tolist():
        fr = np.nonzero(S["id_c"] == c)[0]
        out.append(dict(bins=fr[np.argsort(S["pos"][fr])].tolist(), ring=False, placed=True))
    return out


def _genome(prob, seed=None, ring=False, unplaced=False, single=False, nothing=False, bombed=False):
    """a genome made from the problem's contigs: in the table's order (seed None) or permuted and flipped at random; ``ring``: the
    second contig is a ring; ``unplaced``: the third is not placed; ``single``: the last bin of the first contig is a contig of its
    own; ``bombed``: every bin is"""
    g = _contigs_of(prob)
    if bombed:
        g = [dict(bins=[b], ring=False, placed=True) for c in g for b in c["bins"]]
    if single:
        g.append(dict(bins=[g[0]["bins"].pop()], ring=False, placed=True))
    if ring:
        g[1]["ring"] = True
    if unplaced:
        g[2]["placed"] = False
    if nothing:
        for c in g:
            c["placed"] = False
    if seed is not None:
        rng = np.random.RandomState(seed)
        g = [g[i] for i in rng.permutation(len(g))]
        for c in g:
            if rng.rand() < 0.5:
                c["bins"] = c["bins"][::-1]
                c["flip"] = True
    return g


def _lay_out(prob, genome):
    """-> stot, contig, placed, position, parent, n_bins (what support_host takes in front of the contacts)"""
    parent = prob.np_sub_frags_2_frags["x"].astype(np.int64)
    M = parent.size
    subs = [np.nonzero(parent == b)[0] for b in range(prob.n_frags)]
    stot, contig, placed, position = np.zeros(M, np.float32), np.zeros(M, np.int64), np.ones(M, bool), np.full(M, -1, np.int64)
    at = 0
    for k, c in enumerate(genome):
        for b in c["bins"]:
            s = subs[b][::-1] if c.get("flip") else subs[b]
            contig[s] = k
            if c["ring"]:
                stot[s] = 1.0
            if not c["placed"]:
                placed[s] = False
                continue
            position[s] = at + np.arange(s.size)
            at += s.size
    return stot, contig, placed, position, parent, prob.n_frags


def _contacts(prob):
    return prob.coo_row.astype(np.int64), prob.coo_col.astype(np.int64), prob.coo_cnt.astype(np.int64)


def _exact_best(obs, hosts, ok):
    """the best site by exact integers, another way than the module's: climb to a site nobody is strictly denser than, then the first
    of its equals"""
    idx = np.nonzero(ok & (obs > 0))[0]
    if idx.size == 0:
        return -1
    best = idx[0]
    while True:
        better = idx[obs[idx] * hosts[best] > obs[best] * hosts[idx]]
        if better.size == 0:
            break
        best = better[0]
    return int(idx[obs[idx] * hosts[best] == obs[best] * hosts[idx]][0])


_MASKS = {}


def _masks(n, w):
    """left[u, x], right[u, x]: position x of a contig of n is in the left / right part of the window of site u"""
    if (n, w) not in _MASKS:
        u, x = np.arange(n + 1)[:, None], np.arange(n)[None, :]
        _MASKS[(n, w)] = (((x >= u - w) & (x < u)).astype(np.int64), ((x >= u) & (x < u + w)).astype(np.int64))
    return _MASKS[(n, w)]


def _brute(prob, genome, w, min_hosts_list):
    """the definition on the dense matrix -> {min_hosts: {array name: values}}"""
    from instagraal_amd import placement_support as ps

    stot, contig, placed, position, parent, N = _lay_out(prob, genome)
    row, col, cnt = _contacts(prob)
    M = parent.size
    D = np.zeros((M, M), np.int64)
    np.add.at(D, (row, col), cnt)
    D = D + D.T
    order = np.nonzero(placed)[0]
    order = order[np.argsort(position[order])]
    Dp = D[order][:, order]
    label = np.where(stot[order] != 0, -1, contig[order])  # (contig per position; rings: -1: no site there, no contact from there)
    Dp[label < 0, :] = 0
    Dp[:, label < 0] = 0
    bin_at = parent[order]
    out = {mh: {k: np.zeros(N, np.int32 if k in ps.INT_ARRAYS else np.int64) for k in ps.ARRAYS} for mh in min_hosts_list}
    for mh in min_hosts_list:
        for k in ps.CONTIG_FIELDS:
            out[mh][k][:] = -1
    lin = [k for k, c in enumerate(genome) if c["placed"] and not c["ring"]]
    run_of = {k: i for i, k in enumerate(lin)}
    for k, c in enumerate(genome):
        for b in c["bins"]:
            st = 1 if not c["placed"] else 2 if c["ring"] else 0
            for mh in min_hosts_list:
                out[mh]["status"][b] = st
            if st:
                continue
            mine = np.nonzero(bin_at == b)[0]
            v = np.delete(Dp[mine].sum(axis=0), mine)
            lab = np.delete(label, mine)
            sk, su, left, right, hosts = [], [], [], [], []
            home = None
            for kk in lin:
                where = np.nonzero(lab == kk)[0]
                n = where.size
                if kk == k:
                    uh = int(mine[0] - np.nonzero(label == k)[0][0])
                    if n == 0:
                        home = (uh, 0, 0, 0)
                        continue
                ml, mr = _masks(n, w)
                vk = v[where]
                sk.append(np.full(n + 1, run_of[kk])), su.append(np.arange(n + 1))
                left.append(ml @ vk), right.append(mr @ vk), hosts.append(ml.sum(axis=1) + mr.sum(axis=1))
                if kk == k:
                    home = (uh, int(left[-1][uh]), int(right[-1][uh]), int(hosts[-1][uh]))
            sk, su, left, right, hosts = (np.concatenate(a) if a else np.zeros(0, np.int64) for a in (sk, su, left, right, hosts))
            obs = left + right
            for mh in min_hosts_list:
                o = out[mh]
                o["contig"][b], o["offset"][b], o["n_positions"][b] = run_of[k], home[0], mine.size
                o["home_left"][b], o["home_right"][b], o["home_hosts"][b] = home[1], home[2], home[3]
                ok = (hosts >= mh) & ~((sk == run_of[k]) & (np.abs(su - home[0]) < 2 * w))
                for which in ("best", "second"):
                    i = _exact_best(obs, hosts, ok)
                    if i < 0:
                        break
                    o[which + "_contig"][b], o[which + "_offset"][b], o[which + "_hosts"][b] = sk[i], su[i], hosts[i]
                    o[which + "_left"][b], o[which + "_right"][b] = left[i], right[i]
                    ok = ok & ~((sk == sk[i]) & (np.abs(su - su[i]) < 2 * w))
    return out


STATES = dict(fresh={}, shuffled=dict(seed=5), ring=dict(seed=6, ring=True), unplaced=dict(seed=7, unplaced=True), single=dict(seed=8, single=True),
              all_of_it=dict(seed=9, ring=True, unplaced=True, single=True), nothing=dict(nothing=True))


def _assert_same(got, want, what):
    from instagraal_amd import placement_support as ps

    for k in ps.ARRAYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k, np.nonzero(got[k] != want[k])[0][:5])


@pytest.mark.parametrize("state", sorted(STATES))
def test_the_rule_equals_brute_force_and_the_candidates_suffice_on_tiny(state):
    """support_host (every site) against the dense brute force, and support_sparse (the candidate sites only, through the original
    positions: the device's route) against support_host"""
    from instagraal_amd import placement_support as ps

    prob = _problem()
    genome = _genome(prob, **STATES[state])
    t = _lay_out(prob, genome)
    row, col, cnt = _contacts(prob)
    total = int(cnt.sum())
    for w in WINDOWS:
        mhs = (1, w, 2 * w) if w > 1 else (1, 2)
        want = _brute(prob, genome, w, mhs)
        for mh in mhs:
            got = ps.support_host(*t, row, col, cnt, w, mh)
            _assert_same(got, want[mh], (state, w, mh))
            _assert_same(ps.support_sparse(*t, row, col, cnt, w, mh), got, (state, w, mh, "sparse"))
            # the identities
            assert ps.observed_total(got) == total and got["entries"] % 2 == 0
            assert int(got["count"].sum()) == 2 * got["counted_observed"] and int(got["row_entries"].sum()) == got["entries"]
            assert got["n_guests"] == int((got["status"] == 0).sum()) and got["n_contigs"] == sum(c["placed"] and not c["ring"] for c in genome)
            guest = got["status"] == 0
            for k in ps.ARRAYS[1:]:
                assert np.all(got[k][~guest] == (-1 if k in ps.CONTIG_FIELDS else 0)), k
            has = got["best_contig"] >= 0
            assert np.all(got["best_hosts"][has] >= mh) and np.all((got["best_left"] + got["best_right"])[has] > 0)
            assert np.all(got["second_contig"][~has] == -1)
            if w >= int(got["contig_positions"].max(initial=0)):  # one window per foreign contig, the whole contig: ties pick u = 0
                foreign = has & (got["best_contig"] != got["contig"])
                assert np.all(got["best_offset"][foreign] == 0) and np.all(got["best_left"][foreign] == 0)
                b = np.nonzero(foreign)[0]
                for g in b[:20].tolist():  # obs: the guest's total with that contig
                    k = got["best_contig"][g]
                    lo, hi = got["first_position"][k], got["first_position"][k] + got["contig_positions"][k]
                    c = got["col"][got["rowptr"][g]:got["rowptr"][g + 1]]
                    assert got["best_right"][g] == got["count"][got["rowptr"][g]:got["rowptr"][g + 1]][(c >= lo) & (c < hi)].sum()
        if state == "nothing":
            assert got["n_guests"] == 0 and got["unplaced_observed"] == total and got["entries"] == 0 and np.all(got["status"] == 1)
        if state == "all_of_it":
            assert got["ring_observed"] > 0 and got["unplaced_observed"] > 0 and got["within_bin_observed"] > 0 and 2 in got["status"] and 1 in got["status"]
        if state in ("single", "all_of_it"):  # a contig of one bin, as guest (no home) and as host
            whole = np.nonzero(guest & (got["home_hosts"] == 0))[0]
            assert whole.size == 1 and got["offset"][whole[0]] == 0
            small = ps.support_host(*t, row, col, cnt, 4, 1)
            assert np.any(small["best_contig"] == got["contig"][whole[0]]) or np.any(small["second_contig"] == got["contig"][whole[0]])


def test_no_contacts():
    from instagraal_amd import placement_support as ps

    prob = _problem()
    none = np.zeros(0, np.int64)
    got = ps.support_host(*_lay_out(prob, _genome(prob, seed=3)), none, none, none, 64)
    assert got["n_guests"] == prob.n_frags and got["entries"] == 0 and ps.observed_total(got) == 0
    assert np.all(got["best_contig"] == -1) and np.all(got["contig"] >= 0) and np.all(got["home_hosts"] > 0) and not got["home_left"].any()
    _assert_same(ps.support_sparse(*_lay_out(prob, _genome(prob, seed=3)), none, none, none, 64), got, "sparse")


def _best_of(n, w, mh, x, c, home, exclude, sites):
    """the best of ``sites`` of a hand-made contig with entries at the reduced offsets x with counts c -> (u, obs, hosts) or None"""
    from instagraal_amd import placement_support as ps

    sites = np.asarray(sites, np.int64)
    sites = sites[ps.eligible(n, w, mh, sites, home, exclude)]
    lo, hi = ps.site_window(n, w, sites)
    obs = np.array([int(c[(x >= a) & (x < b)].sum()) for a, b in zip(lo, hi)], np.int64)
    i = _exact_best(obs, hi - lo, np.ones(sites.size, bool))
    return None if i < 0 else (int(sites[i]), int(obs[i]), int(hi[i] - lo[i]))


def test_candidate_sites_hold_the_maximum_on_hand_made_rows():
    """entries at u = 0 and u = n', on both edges of the home exclusion, contigs with n' <= w and w < n' < 2 w, and a random sweep: the
    best over the candidates is the best over every site"""
    from instagraal_amd import placement_support as ps

    cases = []
    for n, w in ((40, 4), (40, 8), (7, 8), (8, 8), (12, 8), (15, 8), (16, 8), (17, 8), (1, 1), (2, 1), (100, 1), (3, 1024)):
        for mh in sorted({1, w, 2 * w, max(1, w - 1), min(2 * w, w + 1)}):
            for home in (None, 0, n, n // 2, 2 * w, n - 2 * w):
                if home is not None and not 0 <= home <= n:
                    continue
                edges = [] if home is None else [home - 2 * w, home - 2 * w - 1, home + 2 * w, home + 2 * w - 1, home - 3 * w, home + 3 * w - 1]
                for x in ([0], [n - 1], [0, n - 1], [e for e in edges if 0 <= e < n], list(range(n)), [n // 2]):
                    if x:
                        cases.append((n, w, mh, np.array(sorted(set(x)), np.int64), home))
    rng = np.random.RandomState(1)
    for _ in range(1500):
        n, w = int(rng.randint(1, 60)), int(rng.randint(1, 12))
        x = np.unique(rng.randint(0, n, rng.randint(1, 8)))
        cases.append((n, w, int(rng.randint(1, 2 * w + 1)), x, None if rng.rand() < 0.4 else int(rng.randint(0, n + 1))))
    rng = np.random.RandomState(2)
    n_best = n_second = 0
    for n, w, mh, x, home in cases:
        c = rng.randint(1, 4, x.size).astype(np.int64)
        every = np.arange(n + 1)
        cand = ps.candidate_sites(n, w, mh, x, home=home)
        assert np.all(np.diff(cand) > 0) and cand.size <= 4 * x.size + 8 and (cand.size == 0 or (cand[0] >= 0 and cand[-1] <= n))
        want = _best_of(n, w, mh, x, c, home, None, every)
        assert _best_of(n, w, mh, x, c, home, None, cand) == want, (n, w, mh, x, c, home)
        if want is None:
            continue
        n_best += 1
        cand2 = ps.candidate_sites(n, w, mh, x, home=home, exclude=want[0])
        assert cand2.size <= 4 * x.size + 10
        second = _best_of(n, w, mh, x, c, home, want[0], every)
        assert _best_of(n, w, mh, x, c, home, want[0], cand2) == second, (n, w, mh, x, c, home, want)
        n_second += second is not None
    assert n_best > 500 and n_second > 50


def test_the_tie_rule_on_a_hand_made_profile():
    """two sites of equal density: the lower (k, u) wins, and the other is the runner-up"""
    from instagraal_amd import placement_support as ps

    # 3 contigs of bins with one sub-fragment each: [0 1 2 3] [4 5 6 7] [8]; the guest 8 has 3 contacts with bin 1 and 3 with bin 5
    parent = np.arange(9)
    contig = np.array([0, 0, 0, 0, 1, 1, 1, 1, 2])
    position = np.arange(9)
    stot, placed = np.zeros(9, np.float32), np.ones(9, bool)
    row, col, cnt = np.array([1, 5, 0]), np.array([8, 8, 1]), np.array([3, 3, 7])
    got = ps.support_host(stot, contig, placed, position, parent, 9, row, col, cnt, 1, 1)
    g = 8
    assert (got["contig"][g], got["offset"][g], got["n_positions"][g], got["home_hosts"][g]) == (2, 0, 1, 0)
    # site (0, 1): left = bin 0 (nothing), right = bin 1 (3): 3 / 2; site (0, 2): left = bin 1: 3 / 2 as well -- the lower u wins
    assert (got["best_contig"][g], got["best_offset"][g], got["best_hosts"][g], got["best_left"][g], got["best_right"][g]) == (0, 1, 2, 0, 3)
    # the runner-up is at least 2 w = 2 sites away or in another contig: (1, 1) beats (0, 3), equal density, lower ... no: (0, 3) has nothing
    assert (got["second_contig"][g], got["second_offset"][g], got["second_left"][g], got["second_right"][g]) == (1, 1, 0, 3)
    one = ps.support_host(stot, contig, placed, position, parent, 9, row, col, cnt, 1, 2)
    assert one["best_offset"][g] == 1 and one["best_hosts"][g] == 2
    # bin 0: its 7 contacts are with its neighbour (home right); elsewhere nothing
    assert (got["home_left"][0], got["home_right"][0], got["home_hosts"][0], got["best_contig"][0]) == (0, 7, 1, -1)
    d = ps.densities(got)
    assert d["ratio"][g] == np.inf and d["home_density"][g] == 0 and d["best_density"][g] == 1.5 and d["second_ratio"][g] == 1.0
    assert d["ratio"][0] == 0.0 and np.isnan(d["second_ratio"][0]) and np.isnan(d["ratio"][2])  # (bin 2: no contact at all)
    _assert_same(ps.support_sparse(stot, contig, placed, position, parent, 9, row, col, cnt, 1, 1), got, "sparse")


def test_arguments_and_the_overflow_guard():
    from instagraal_amd import placement_support as ps

    prob = _problem()
    t = _lay_out(prob, _genome(prob))
    row, col, cnt = _contacts(prob)
    for bad in (0, 1025, 2.5):
        with pytest.raises(ValueError, match="window"):
            ps.support_host(*t, row, col, cnt, bad)
    for w, bad in ((4, 0), (4, 9), (1, 3), (4, 1.5)):
        with pytest.raises(ValueError, match="min_hosts"):
            ps.support_host(*t, row, col, cnt, w, bad)
    big = cnt.copy()
    big[0] = (1 << 62) // (2 * 64)  # 2 w sum >= 2^62
    with pytest.raises(ValueError, match="counts too large for this window"):
        ps.support_host(*t, row, col, big, 64)
    assert ps.support_host(*t, row, col, big, 1)["counted_observed"] + ps.support_host(*t, row, col, big, 1)["within_bin_observed"] > 1 << 50


def _result_table():
    """a hand-made result of six bins for the ranking and the file"""
    from instagraal_amd import placement_support as ps

    N = 6
    r = {k: np.zeros(N, np.int32 if k in ps.INT_ARRAYS else np.int64) for k in ps.ARRAYS}
    r["status"][:] = [0, 0, 0, 0, 1, 0]
    r["contig"][:] = [0, 0, 1, 1, -1, 2]
    r["n_positions"][:] = [1, 2, 1, 1, 0, 1]
    r["home_hosts"][:] = [4, 4, 4, 4, 0, 0]
    r["home_left"][:] = [4, 2, 1, 8, 0, 0]
    r["best_contig"][:] = [1, 1, 0, -1, -1, 0]
    r["best_offset"][:] = [1, 0, 2, 0, 0, 1]
    r["best_hosts"][:] = [4, 2, 4, 0, 0, 2]
    r["best_right"][:] = [8, 4, 2, 0, 0, 5]  # ratios: 2, 2 (of two positions: 1 / 0.25 ... see below), 2, nan -> 0, nan, inf
    r["second_contig"][:] = [-1, -1, 1, -1, -1, -1]
    r["second_hosts"][:] = [0, 0, 4, 0, 0, 0]
    r["second_left"][:] = [0, 0, 1, 0, 0, 0]
    r.update(ps.densities(r))
    r.update(window=2, min_hosts=2, scaffold=np.array([3, 3, 4, 4, -1, 5]), offset=np.array([0, 1, 0, 1, 0, 0], np.int32))
    r.update(best_scaffold=np.array([4, 4, 3, -1, -1, 3]), best_before=np.array([2, -1, 1, -1, -1, 0]), best_after=np.array([3, 2, -1, -1, -1, 1]))
    r.update({k: i for i, k in enumerate(ps.SCALARS)})
    return r


def test_the_ranking_and_the_file(tmp_path):
    from instagraal_amd import placement_support as ps

    r = _result_table()
    assert r["ratio"][:4].tolist() == [2.0, 4.0, 2.0, 0.0] and np.isnan(r["ratio"][4]) and r["ratio"][5] == np.inf
    assert r["second_ratio"][2] == 0.5 and r["second_ratio"][0] == 0.0 and np.isnan(r["second_ratio"][3])
    t = ps.misplaced_bins(r)
    assert t["bin"].tolist() == [5, 1, 0, 2] and t.dtype == ps.PLACEMENT_DTYPE  # inf first, ties by bin id
    assert ps.misplaced_bins(r, n=2)["bin"].tolist() == [5, 1] and ps.misplaced_bins(r, min_ratio=2.0)["bin"].tolist() == [5, 1]
    assert ps.misplaced_bins(r, n=0).size == 0 and ps.misplaced_bins(r, min_ratio=-1.0)["bin"].tolist() == [5, 1, 0, 2]  # (no best site: never listed)
    assert t["best_scaffold"].tolist() == [3, 4, 4, 3] and t["ratio"].tolist() == [np.inf, 4.0, 2.0, 2.0]
    path = str(tmp_path / "placements.txt")
    assert ps.write_placements(path, r) == 4
    lines = open(path).read().splitlines()
    assert lines[0][2:].split() == list(ps.PLACEMENT_COLUMNS) and len(lines) == 6
    rows = [ln.split() for ln in lines[1:-1]]
    assert [int(x[0]) for x in rows] == [5, 1, 0, 2] and rows[0][10] == "inf" and all(len(x) == len(ps.PLACEMENT_COLUMNS) for x in rows)
    assert rows[1][7] == "-" and rows[1][8] == "2" and rows[3][8] == "-" and rows[0][1].endswith("5") and rows[0][5].endswith("3")
    sc = dict(kv.split("=") for kv in lines[-1][2:].split())
    assert int(sc["window"]) == 2 and int(sc["min_hosts"]) == 2 and [int(sc[k]) for k in ps.SCALARS] == list(range(7))
    assert ps.write_placements(path, r, n=1) == 1 and len(open(path).read().splitlines()) == 3


def _plant(genome):
    """the middle bin of the longest contig moved to the tail of the second longest -> (genome, bin, the contig it came from, its
    former reduced offset in sub-fragments is left to the caller)"""
    by_len = sorted(range(len(genome)), key=lambda k: -len(genome[k]["bins"]))
    a, b = by_len[0], by_len[1]
    g = [dict(c, bins=list(c["bins"])) for c in genome]
    mid = (len(g[a]["bins"]) - 1) // 2  # (of an even number of bins the lower middle: the one whose offsets the feature was first measured at)
    moved = g[a]["bins"].pop(mid)
    g[b]["bins"].append(moved)
    return g, moved, a, mid


@pytest.mark.parametrize("cfg,w", [("tiny", 4), ("small", 8), ("small", 32)])
def test_the_planted_misplacement_is_the_one_bin_flagged(cfg, w):
    from instagraal_amd import placement_support as ps

    prob = _problem(cfg)
    row, col, cnt = _contacts(prob)
    genome = _genome(prob)
    fresh = ps.support_host(*_lay_out(prob, genome), row, col, cnt, w)
    assert not np.any(ps.densities(fresh)["ratio"] > 1)  # nowhere denser than at home
    planted, moved, came_from, mid = _plant(genome)
    t = _lay_out(prob, planted)
    got = ps.support_host(*t, row, col, cnt, w)
    ratio = ps.densities(got)["ratio"]
    assert np.nonzero(ratio > 1)[0].tolist() == [moved] and got["home_left"][moved] + got["home_right"][moved] == 0
    parent = t[4]
    former = sum(int((parent == b).sum()) for b in planted[came_from]["bins"][:mid])  # the reduced offset it was taken from
    assert got["best_contig"][moved] == came_from and abs(int(got["best_offset"][moved]) - former) <= w
    assert np.nanmax(np.where(np.arange(ratio.size) == moved, np.nan, ratio)) < 1.0
    _assert_same(ps.support_sparse(*t, row, col, cnt, w), got, "sparse")
    # the translation for people, on tables made by hand from the same layout
    order = np.argsort(np.where(t[3] >= 0, t[3], 1 << 40), kind="stable")[:int((t[3] >= 0).sum())]
    names = ps.sites_for_people(got, order, parent, np.asarray(t[1])[[np.nonzero(parent == b)[0][0] for b in range(prob.n_frags)]])
    bins = planted[came_from]["bins"]
    u = int(got["best_offset"][moved])
    flat = [b for b in bins for _ in range(int((parent == b).sum()))]
    assert names["best_scaffold"][moved] == came_from and names["scaffold"][moved] == got["contig"][moved]
    assert names["best_before"][moved] == (flat[u - 1] if u else -1) and names["best_after"][moved] == (flat[u] if u < len(flat) else -1)


def test_the_preconditions_of_the_gpu_tests():
    """the states tests/test_hip_placement_support.py compares on: rows on both sides of PLACE_WAVE_ENTRIES, best sites in the clipped
    zone at a head and at a tail, rows without an eligible site, a guest that is a whole contig"""
    from instagraal_amd import placement_support as ps

    src = open(os.path.join(ROOT, "instagraal_amd", "csrc", "ig_kernels_place.cuh")).read()
    assert "#define PLACE_WAVE_ENTRIES %d\n" % ps.WAVE_ENTRIES in src
    prob = _problem("small")
    row, col, cnt = _contacts(prob)
    t = _lay_out(prob, _genome(prob))
    got = ps.support_host(*t, row, col, cnt, 64, 1)
    n = np.diff(got["rowptr"])
    assert (n <= ps.WAVE_ENTRIES).sum() > 50 and (n > ps.WAVE_ENTRIES).sum() > 50
    has = got["best_contig"] >= 0
    n_red = got["contig_positions"][np.maximum(got["best_contig"], 0)] - np.where(got["best_contig"] == got["contig"], got["n_positions"], 0)
    assert np.any(has & (got["best_offset"] < 64) & (got["best_hosts"] < 128)) and np.any(has & (got["best_offset"] > n_red - 64) & (got["best_hosts"] < 128))
    wide = ps.support_host(*t, row, col, cnt, 1024, 2048)
    assert not np.any(wide["best_contig"] >= 0) and wide["n_guests"] == prob.n_frags  # no contig of 2048 positions: no eligible site
    bombed = ps.support_host(*_lay_out(prob, _genome(prob, bombed=True)), row, col, cnt, 64, 1)
    assert np.all(bombed["home_hosts"] == 0) and np.all(bombed["status"] == 0) and (bombed["best_contig"] >= 0).sum() > 900
    tiny = _problem("tiny")
    assert np.diff(ps.support_host(*_lay_out(tiny, _genome(tiny)), *_contacts(tiny), 64)["rowptr"]).max() <= ps.WAVE_ENTRIES  # (the forced forms reach them)


def test_the_module_imports_without_a_gpu_library():
    code = ("import instagraal_amd.placement_support as p, instagraal_amd.sampler, instagraal_amd.simulation, instagraal_amd.hip_lib as h\n"
            "assert h._lib is None and len(h.PLACEMENT_SUPPORT_PASSES) == 10 and len(p.SCALARS) == 7\n")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)
