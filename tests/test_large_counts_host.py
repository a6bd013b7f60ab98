"""CPU tests of the large-count problems of tests/_large_counts.py and of the rules at counts up to 2^31 - 1.

* the inputs reach the segmented wave scans of the three observed passes: on the fresh genome a run of 64 equal destinations fills an
  aligned block of 64 consecutive contacts, and its counts sum to exactly 2^31 - 64 (the last sum an `int` holds), to 2^31, and to
  64 (2^31 - 1);
* every numpy rule the device passes are held against, once against a brute-force statement in Python integers on a reduced
  `int_max` list: the rule itself neither wraps nor rounds;
* ``hip_lib.as_int32_exact``, the check in front of ``upload_contacts``.

Everything is exact integer equality."""
import numpy as np
import pytest

import _large_counts as lc

W_RUN = 256  # the window at which a dense row's 192 contacts are all in window


@pytest.fixture(scope="module")
def cfg():
    name = lc.smallest_config()
    assert lc.longest_contig(lc._synth(name))[1] >= 200 + 8
    return name


def test_the_lists_are_sorted_distinct_and_upper_triangular(cfg):
    base = lc.make(cfg, "base")
    M = base.n_sub_frags
    for family in lc.FAMILIES:
        p = lc.make(cfg, family)
        key = p.coo_row.astype(np.int64) * M + p.coo_col
        assert np.all(np.diff(key) > 0) and np.all(p.coo_row < p.coo_col) and p.coo_cnt.dtype == np.int32 and p.coo_cnt.min() >= 1
        csr = p.sub_csr.tocoo()
        assert np.array_equal(csr.row, p.coo_row) and np.array_equal(csr.col, p.coo_col) and np.array_equal(csr.data, p.coo_cnt)
        if family != "one_wide":
            assert np.array_equal(p.coo_row, base.coo_row) and np.array_equal(p.coo_col, base.coo_col)
    synth = lc._synth(cfg)
    one = lc.make(cfg, "one_wide")
    changed = np.nonzero(one.coo_cnt != synth.coo_cnt)[0]
    c_of = synth.S_o_A_sub_frags["id_c"]
    assert changed.size == 1 and one.coo_cnt[changed[0]] == 2 ** 25 and c_of[one.coo_row[changed[0]]] != c_of[one.coo_col[changed[0]]]
    assert synth.coo_cnt.max() < 2 ** 24 and np.array_equal(one.coo_row, synth.coo_row)
    assert [int(lc.make(cfg, f).coo_cnt.max()) for f in ("base", "narrow_max", "wide_min", "int_max")] == [int(synth.coo_cnt.max()), 2 ** 25 - 1, 2 ** 25, 2 ** 31 - 1]
    im = lc.make(cfg, "int_max")
    assert (im.coo_cnt == lc.INT_MAX).sum() >= lc.N_DENSE * lc.DENSE_LEN + (im.coo_cnt.size - lc.N_DENSE * lc.DENSE_LEN) // 7


def test_wave_stats_on_hand_made_lists():
    d = np.array([5] * 70 + [-1] * 58 + [7] * 64)  # blocks: 64 x 5 | 6 x 5, 58 x none | 64 x 7
    c = np.arange(1, d.size + 1)
    assert lc.wave_stats(d, c) == (64, sum(range(129, 193)))
    assert lc.wave_stats(d[:128], c[:128]) == (64, sum(range(1, 65)))
    assert lc.wave_stats(np.r_[np.full(32, -1), np.full(64, 3)], np.full(96, lc.INT_MAX)) == (32, 32 * lc.INT_MAX)  # a run across two blocks is two runs
    assert lc.wave_stats(np.full(10, -1), np.ones(10)) == (0, 0) and lc.wave_stats([], []) == (0, 0)
    assert lc.wave_stats(np.zeros(64), np.full(64, lc.INT_MAX)) == (64, 64 * lc.INT_MAX)


def _destinations(p):
    """the per-contact destination arrays of the three combining passes on the fresh genome -> {name: array}"""
    first, last = lc.dense_segments(p)
    out = {"map key, max_side %d" % m: lc.map_keys(p, m) for m in (1, 2)}
    out["junction + word, window %d" % W_RUN] = lc.junction_plus_words(p, W_RUN)
    out["orientation row-end word, window %d" % W_RUN] = lc.orientation_row_words(p, first, last, W_RUN)
    return out


def test_a_full_run_of_64_lanes_exists_for_every_combining_pass(cfg):
    """the map key at max_side 1 and 2, the junction profile's + word and the orientation support's row-end word (quadrant RR of the
    segments that end at the dense rows).  With one sub-fragment per pixel the contacts of a distinct list all have different keys:
    no two lanes can share one, every lane is a run head and the pass takes the branch that skips the scan -- that is what is shown
    for it."""
    for family in ("base", "narrow_max", "wide_min", "int_max"):
        p = lc.make(cfg, family)
        for name, dest in _destinations(p).items():
            assert lc.wave_stats(dest, p.coo_cnt)[0] == 64, (family, name)
        first, last = lc.dense_segments(p)
        words = lc.orientation_row_words(p, first, last, W_RUN)
        dense = np.isin(p.coo_row, lc.dense_rows(p)) & (p.coo_col - p.coo_row <= lc.DENSE_LEN)
        assert dense.sum() == lc.N_DENSE * lc.DENSE_LEN
        assert np.array_equal(words[dense], np.repeat(4 * np.arange(lc.N_DENSE) + 3, lc.DENSE_LEN))  # every dense contact: RR of its segment
        per_pixel = lc.map_keys(p, p.n_sub_frags)
        assert np.unique(per_pixel).size == per_pixel.size and lc.wave_stats(per_pixel, p.coo_cnt)[0] == 1


def test_the_largest_sum_of_a_run_inside_a_wave(cfg):
    """narrow_max: exactly 2^31 - 64, the last sum that fits an int; wide_min: exactly 2^31; int_max: 64 (2^31 - 1) = 2^37 - 64, the
    largest sum 64 lanes of int32 counts can have (beyond 2^36: 38 bits)"""
    want = dict(narrow_max=2 ** 31 - 64, wide_min=2 ** 31, int_max=64 * (2 ** 31 - 1))
    assert want["int_max"] == 2 ** 37 - 64 and want["int_max"] > 2 ** 36
    for family, total in want.items():
        p = lc.make(cfg, family)
        for name, dest in _destinations(p).items():
            assert lc.wave_stats(dest, p.coo_cnt) == (64, total), (family, name)
    assert np.iinfo(np.int32).max - (2 ** 31 - 64) == 63 and 2 ** 31 > np.iinfo(np.int32).max


# ---- the rules against Python integers


def _reduced(cfg, every=40):
    """`int_max` cut to about a thousand contacts -- three of the dense rows whole, every 40th of the other contacts --, on tables of
    a genome with one contig not placed and one ring, neither the dense rows' contig"""
    p = lc.make(cfg, "int_max")
    rows = lc.dense_rows(p)
    dense = np.isin(p.coo_row, rows) & (p.coo_col - p.coo_row <= lc.DENSE_LEN)
    rest = np.nonzero(~dense)[0]
    keep = np.sort(np.concatenate([np.nonzero(dense & np.isin(p.coo_row, rows[::3]))[0], rest[::every]]))
    row, col, cnt = p.coo_row[keep].astype(np.int64), p.coo_col[keep].astype(np.int64), p.coo_cnt[keep].astype(np.int64)
    assert 800 < keep.size < 1500 and (cnt == lc.INT_MAX).sum() > 600 and (cnt < 1000).sum() > 300
    assert 2 ** 40 < int(cnt.sum()) < 1 << 53  # (no float64 bincount of these counts can round)
    M = p.n_sub_frags
    contig = np.asarray(p.S_o_A_sub_frags["id_c"], np.int64)
    parent = p.np_sub_frags_2_frags["x"].astype(np.int64)
    kb = np.asarray(p.S_o_A_sub_frags["len_bp"], np.float64) / 1000.0
    ids, first, n_of = np.unique(contig, return_index=True, return_counts=True)
    cum = np.cumsum(kb) - kb
    dist = (cum - np.repeat(cum[first], n_of) + kb / 2).astype(np.float32)
    long_first, _ = lc.longest_contig(p)
    ring_c, lost_c = ids[0], ids[-1]
    assert contig[long_first] not in (ring_c, lost_c) and ring_c != lost_c
    stot = np.where(contig == ring_c, np.float32(kb[contig == ring_c].sum()), np.float32(0)).astype(np.float32)
    placed = contig != lost_c
    position = np.where(placed, np.arange(M), -1).astype(np.int64)  # (the contig that is not placed is the last)
    l_cont_bp = np.asarray(p.S_o_A_frags["l_cont_bp"], np.int64)[parent]
    t = dict(dist=dist, stot=stot, contig=contig, placed=placed, position=position, parent=parent, l_cont_bp=l_cont_bp, n_bins=p.n_frags, M=M,
             T=int(placed.sum()), row=row, col=col, cnt=cnt, total=sum(cnt.tolist()), params=p.params)
    klass = []
    for r, c in zip(row.tolist(), col.tolist()):
        if not (placed[r] and placed[c]):
            klass.append("unplaced")
        elif contig[r] != contig[c]:
            klass.append("ring_trans" if (stot[r] != 0 or stot[c] != 0) else "trans")
        else:
            klass.append("ring" if stot[r] != 0 else "lin")
    t["klass"] = klass
    assert {"unplaced", "trans", "ring", "lin", "ring_trans"} <= set(klass)
    return t


@pytest.fixture(scope="module")
def red(cfg):
    return _reduced(cfg)


def _contacts(t):
    return zip(t["row"].tolist(), t["col"].tolist(), t["cnt"].tolist(), t["klass"])


def _ints(a):
    return [int(x) for x in np.asarray(a).ravel().tolist()]


def test_contact_map_rule(red):
    t = red
    pos = t["position"].tolist()
    for max_side in (1, 2, 37, t["T"]):
        from instagraal_amd.contact_map import binning

        b, side = binning(t["T"], max_side)
        want = [[0] * side for _ in range(side)]
        for r, c, v, _ in _contacts(t):
            if pos[r] >= 0 and pos[c] >= 0:
                want[pos[r] // b][pos[c] // b] += v
                want[pos[c] // b][pos[r] // b] += v
        got, gb = lc.map_host(t["position"], t["row"], t["col"], t["cnt"], max_side)
        assert gb == b and got.dtype == np.int64 and got.tolist() == want
        assert sum(map(sum, want)) == 2 * sum(v for _, _, v, k in _contacts(t) if k != "unplaced") > 2 ** 38


def test_distance_law_rule(red):
    from instagraal_amd import distance_law as dl

    t = red
    edges = dl.default_edges(1.8, 900.0, per_octave=3)[:-4]  # (some pairs beyond the last edge)
    got = dl.law_host(t["dist"], t["stot"], t["contig"], t["placed"], t["row"], t["col"], t["cnt"], edges, pairs=False)
    e = [float(x) for x in got["edges"]]
    want = dict(observed=[0] * (len(e) - 1), out_of_range_observed=0, trans_observed=0, ring_observed=0, unplaced_observed=0)
    for r, c, v, k in _contacts(t):
        if k == "unplaced":
            want["unplaced_observed"] += v
        elif k in ("trans", "ring_trans"):
            want["trans_observed"] += v
        elif k == "ring":
            want["ring_observed"] += v
        else:
            s = float(np.abs(t["dist"][r] - t["dist"][c]))  # (an f32 difference; the comparisons with the f32 edges are exact in doubles)
            b = [i for i in range(len(e) - 1) if e[i] <= s < e[i + 1]]
            if b:
                want["observed"][b[-1]] += v
            else:
                want["out_of_range_observed"] += v
    assert _ints(got["observed"]) == want["observed"] and all(got[k] == want[k] for k in dl.OBSERVED_SCALARS)
    assert dl.observed_total(got) == t["total"] and max(want["observed"]) > 2 ** 32 and want["out_of_range_observed"] > 0


def test_junction_profile_rule(red):
    from instagraal_amd import junction_profile as jp

    t = red
    pos = t["position"].tolist()
    for w in (1, 64, W_RUN, 1024):
        got = jp.profile_host(t["dist"], t["stot"], t["contig"], t["placed"], t["position"], t["row"], t["col"], t["cnt"], w)  # (raises if its 2^53 guard fires)
        obs = [0] * t["T"]
        sc = dict.fromkeys(jp.OBSERVED_SCALARS, 0)
        for r, c, v, k in _contacts(t):
            if k != "lin":
                sc[{"unplaced": "unplaced_observed", "trans": "trans_observed", "ring_trans": "trans_observed", "ring": "ring_observed"}[k]] += v
                continue
            pa, pb = min(pos[r], pos[c]), max(pos[r], pos[c])
            if pb - pa > w:
                sc["beyond_window_observed"] += v
                continue
            sc["in_window_observed"] += v
            for j in range(pa + 1, pb + 1):
                obs[j] += v
        assert _ints(got["observed"]) == obs and all(got[k] == sc[k] for k in sc), w
        assert got["spanned_observed"] == sum(obs) and jp.observed_total(got) == t["total"]
        if w >= 64:
            assert max(obs) > 2 ** 32


def test_orientation_support_rule(red):
    from instagraal_amd import orientation_support as osup

    t = red
    pos = t["position"].tolist()
    order = np.nonzero(t["placed"])[0]
    bins = osup.bin_segments(order, t["parent"])
    rows = lc.dense_rows(lc._synth(lc.smallest_config()))
    lists = dict(bin=(bins["first"], bins["last"]), dense=(rows - 1, rows))
    largest = 0
    for name, (first, last) in lists.items():
        for w in (8, W_RUN):
            got = osup.support_host(t["dist"], t["stot"], t["contig"], t["placed"], t["position"], t["row"], t["col"], t["cnt"], first, last, w)
            f, l = _ints(got["first"]), _ints(got["last"])
            judged, arm = (got["geometry"][:, 0] == 0).tolist(), _ints(got["geometry"][:, 1])
            seg = [-1] * t["T"]
            for s, (a, b) in enumerate(zip(f, l)):
                for r in range(a, b + 1):
                    seg[r] = s
            obs = [[0, 0, 0, 0] for _ in f]
            sc = dict.fromkeys(osup.CLASS_SCALARS, 0)
            for r, c, v, k in _contacts(t):
                if k != "lin":
                    sc[{"unplaced": "unplaced", "trans": "trans", "ring_trans": "trans", "ring": "ring"}[k]] += v
                    continue
                pa, pb = min(pos[r], pos[c]), max(pos[r], pos[c])
                sa, sb = seg[pa], seg[pb]
                if sa >= 0 and sa == sb:
                    sc["within_segment"] += v
                    continue
                hits = 0
                if sa >= 0 and judged[sa] and pb - l[sa] <= w:
                    if pa < f[sa] + arm[sa]:
                        obs[sa][osup.LR] += v
                        hits += 1
                    if pa > l[sa] - arm[sa]:
                        obs[sa][osup.RR] += v
                        hits += 1
                if sb >= 0 and judged[sb] and f[sb] - pa <= w:
                    if pb < f[sb] + arm[sb]:
                        obs[sb][osup.LL] += v
                        hits += 1
                    if pb > l[sb] - arm[sb]:
                        obs[sb][osup.RL] += v
                        hits += 1
                sc["counted" if hits else "uncounted"] += v
            assert got["observed"].tolist() == obs and all(got[k] == sc[k] for k in sc), (name, w)
            assert got["entries_observed"] == sum(map(sum, obs)) and osup.observed_total(got) == t["total"]
            largest = max(largest, max(map(max, obs)))
    assert largest > 2 ** 32


def _gap_model(t):
    from instagraal_amd import hip_lib
    from instagraal_amd.sampler import PARAM_NAMES

    hip_lib.build_lib()
    p8 = np.array([np.float32(t["params"][k]) for k in PARAM_NAMES], np.float32)
    return lambda s: hip_lib.model_values_host(p8, s)


def _gap_brute(t, junc, gaps, w, model):
    pos = t["position"].tolist()
    K = len(gaps)
    listed = set(junc)
    obs, logq = {j: 0 for j in junc}, {j: [0] * K for j in junc}
    sc = dict.fromkeys(("unplaced", "trans", "ring", "counted", "uncounted", "contributions"), 0)
    max_l = 0
    for r, c, v, k in _contacts(t):
        if k != "lin":
            sc[{"unplaced": "unplaced", "trans": "trans", "ring_trans": "trans", "ring": "ring"}[k]] += v
            continue
        pa, pb = min(pos[r], pos[c]), max(pos[r], pos[c])
        span = [j for j in range(pa + 1, pb + 1) if j in listed] if pb - pa <= w else []
        sc["counted" if span else "uncounted"] += v
        sc["contributions"] += len(span)
        if span:
            s = np.abs(t["dist"][r] - t["dist"][c])
            lq = _ints(model((s + np.asarray(gaps, np.float32)).astype(np.float32))[1])
            max_l = max(max_l, max(abs(x) for x in lq))
            for j in span:
                obs[j] += v
                logq[j] = [a + v * x for a, x in zip(logq[j], lq)]
    return [obs[j] for j in junc], [logq[j] for j in junc], sc, max_l


def _signed64(x):
    x %= 1 << 64
    return x - (1 << 64) if x >= 1 << 63 else x


def test_gap_support_rule(red):
    """under `int_max` the products count * l_q leave 64 bits: the rule refuses as the device does (the second guard), and with
    ``check=False`` its words are the true sums modulo 2^64; with the large counts at 2^19 it equals the Python integers"""
    from instagraal_amd import gap_support as gs, junction_profile as jp

    t = red
    model = _gap_model(t)
    _, start, length = jp.contig_runs(t["contig"], t["position"])
    ring_pos = t["stot"][np.nonzero(t["placed"])[0]] != 0
    junc = [j for st, n in zip(start.tolist(), length.tolist()) for j in range(st + 1, st + n, 3) if not ring_pos[j]]
    gaps = np.array([0.0, 0.5, 3.0, 40.0, 1000.0], np.float32)
    args = (t["dist"], t["stot"], t["contig"], t["placed"], t["position"], t["row"], t["col"])
    for w in (64, 256):
        obs, logq, sc, max_l = _gap_brute(t, junc, gaps.tolist(), w, model)
        assert max(obs) * max_l >= 1 << 62 and max(abs(x) for row in logq for x in row) >= 1 << 63
        with pytest.raises(ValueError, match="too many contacts across one junction"):
            gs.support_host(*args, t["cnt"], junc, gaps, w, model, want_expected=False)
        got = gs.support_host(*args, t["cnt"], junc, gaps, w, model, want_expected=False, check=False)
        assert _ints(got["observed"]) == obs and all(got[k] == sc[k] for k in sc) and got["max_abs_log_q"] == max_l
        assert got["log_q"].tolist() == [[_signed64(x) for x in row] for row in logq]
        assert not gs.log_sum_fits(max(obs), max_l) and gs.observed_total(got) == t["total"]
        small = dict(t, cnt=np.where(t["cnt"] == lc.INT_MAX, 2 ** 19, t["cnt"]))
        obs, logq, sc, max_l = _gap_brute(small, junc, gaps.tolist(), w, model)
        got = gs.support_host(*args, small["cnt"], junc, gaps, w, model, want_expected=False)
        assert _ints(got["observed"]) == obs and got["log_q"].tolist() == logq and all(got[k] == sc[k] for k in sc)
        assert gs.log_sum_fits(max(obs), max_l) and max(abs(x) for row in logq for x in row) > 2 ** 56


def _linear_runs(t):
    """[(start, n)] of the placed contigs that are not rings, in genome order, and the run of every position (-1: ring)"""
    from instagraal_amd import junction_profile as jp

    members, start, length = jp.contig_runs(t["contig"], t["position"])
    runs, run_of = [], [-1] * t["T"]
    for st, n in zip(start.tolist(), length.tolist()):
        if t["stot"][members[st]] == 0:
            for r in range(st, st + n):
                run_of[r] = len(runs)
            runs.append((st, n))
    return runs, run_of


def test_join_support_rule(red):
    from instagraal_amd import join_support as js

    t = red
    pos = t["position"].tolist()
    runs, run_of = _linear_runs(t)
    for w in (64, 1024):
        got = js.support_host(t["dist"], t["stot"], t["contig"], t["placed"], t["position"], t["l_cont_bp"], t["row"], t["col"], t["cnt"], w)
        links = {}
        sc = dict.fromkeys(js.SCALARS[:6], 0)
        for r, c, v, k in _contacts(t):
            if k != "trans":
                sc[{"unplaced": "unplaced_observed", "ring_trans": "ring_observed", "ring": "ring_observed", "lin": "cis_observed"}[k]] += v
                continue
            pa, pb = pos[r], pos[c]
            ka, kb = run_of[pa], run_of[pb]
            da = (pa - runs[ka][0], runs[ka][0] + runs[ka][1] - 1 - pa)
            db = (pb - runs[kb][0], runs[kb][0] + runs[kb][1] - 1 - pb)
            n = 0
            for sa in (0, 1):
                for sb in (0, 1):
                    if da[sa] + db[sb] + 1 <= w:
                        ea, eb = 2 * ka + sa, 2 * kb + sb
                        links[(min(ea, eb), max(ea, eb))] = links.get((min(ea, eb), max(ea, eb)), 0) + v
                        n += 1
            sc["in_reach_observed" if n else "out_of_reach_observed"] += v
            sc["contributions"] += n * v
        keys = sorted(links)
        assert list(zip(js.rows_of(got["rowptr"]).tolist(), got["col"].tolist())) == keys and _ints(got["observed"]) == [links[k] for k in keys], w
        assert all(got[k] == sc[k] for k in sc) and js.observed_total(got) == t["total"] and sum(links.values()) == sc["contributions"]
        assert got["n_links"] == len(keys) and (w == 64 or (len(keys) > 20 and sc["contributions"] > 2 ** 36 and max(links.values()) > 2 ** 32))


def test_assembly_contacts_rule(red):
    from instagraal_amd import assembly_contacts as ac

    t = red
    pos = t["position"].tolist()
    order = np.nonzero(t["placed"])[0]
    unit = ac.units_along(t["parent"][order])
    for level, of in (("sub", None), ("bin", unit)):
        got = ac.lift_host(t["position"], t["row"], t["col"], t["cnt"], unit=of)
        key = pos if of is None else [int(of[p]) if p >= 0 else -1 for p in pos]
        cells, lost = {}, 0
        for r, c, v, _ in _contacts(t):
            a, b = key[r], key[c]
            if a < 0 or b < 0:
                lost += v
            else:
                cells[(min(a, b), max(a, b))] = cells.get((min(a, b), max(a, b)), 0) + v
        keys = sorted(cells)
        assert list(zip(ac.rows_of(got["rowptr"]).tolist(), got["col"].tolist())) == keys and _ints(got["count"]) == [cells[k] for k in keys], level
        assert got["contacts_unplaced"] == lost > 0 and got["contacts_kept"] == sum(cells.values()) == t["total"] - lost and got["entries_out"] == len(keys)
    assert max(cells.values()) > 2 ** 32  # (level bin: equal cells summed)


def test_balance_entries_rule(red):
    from instagraal_amd import assembly_contacts as ac, balance as bal

    t = red
    order = np.nonzero(t["placed"])[0]
    unit = ac.units_along(t["parent"][order])
    for level, kw, diags in (("sub", {}, 1), ("bin", dict(unit=unit), 2), ("map", dict(max_side=16), 2), ("map", dict(max_side=3), 1)):
        key, U = bal.keys_of(t["position"], level, **kw)
        got = bal.entries_host(key, U, t["row"], t["col"], t["cnt"], ignore_diags=diags)  # (raises if a total reaches 2^53)
        k_of = key.tolist()
        cells = {}
        sc = dict.fromkeys(bal.OBSERVED_SCALARS, 0)
        for r, c, v, _ in _contacts(t):
            a, b = k_of[r], k_of[c]
            if a < 0 or b < 0:
                sc["unplaced_observed"] += v
            elif a == b:
                sc["within_observed"] += v
            elif abs(a - b) < diags:
                sc["band_observed"] += v
            else:
                sc["kept_observed"] += v
                for x in ((a, b), (b, a)):
                    cells[x] = cells.get(x, 0) + v
        keys = sorted(cells)
        assert list(zip(ac.rows_of(got["rowptr"]).tolist(), got["col"].tolist())) == keys and _ints(got["count"]) == [cells[k] for k in keys], level
        total = [sum(v for (a, _), v in cells.items() if a == u) for u in range(U)]
        assert _ints(got["total"]) == total and _ints(got["nnz"]) == [sum(1 for (a, _) in cells if a == u) for u in range(U)]
        assert all(got[k] == sc[k] for k in sc) and bal.observed_total(got) == t["total"] and sum(total) == 2 * sc["kept_observed"]
        assert max(total) > 2 ** 32 and max(total) < bal.MAX_TOTAL


def _better(x, y):
    """site x = (obs, hosts, k, u) beats y: denser by exact integers, on equality the lower (k, u)"""
    if y is None:
        return True
    lhs, rhs = x[0] * y[1], y[0] * x[1]
    return lhs > rhs or (lhs == rhs and (x[2], x[3]) < (y[2], y[3]))


def test_placement_support_rule(red):
    from instagraal_amd import placement_support as ps

    t = red
    pos, parent = t["position"].tolist(), t["parent"].tolist()
    runs, run_of = _linear_runs(t)
    w, mh = 8, 8
    got = ps.support_host(t["stot"], t["contig"], t["placed"], t["position"], t["parent"], t["n_bins"], t["row"], t["col"], t["cnt"], w)
    sc = dict.fromkeys(ps.OBSERVED_SCALARS, 0)
    rows = {}  # bin -> {position: count}
    n_counted = 0
    for r, c, v, k in _contacts(t):
        if k == "unplaced":
            sc["unplaced_observed"] += v
        elif k in ("ring", "ring_trans"):
            sc["ring_observed"] += v
        elif parent[r] == parent[c]:
            sc["within_bin_observed"] += v
        else:
            sc["counted_observed"] += v
            n_counted += 1
            for g, p in ((parent[r], pos[c]), (parent[c], pos[r])):
                rows.setdefault(g, {})
                rows[g][p] = rows[g].get(p, 0) + v
    assert all(got[k] == sc[k] for k in sc) and ps.observed_total(got) == t["total"] and got["entries"] == 2 * n_counted
    assert sum(sum(r.values()) for r in rows.values()) == 2 * sc["counted_observed"] > 2 ** 40
    of_bin = {}
    for s, p in enumerate(pos):
        if p >= 0 and run_of[p] >= 0:
            of_bin.setdefault(parent[s], []).append(p)
    moved = 0
    for g in range(t["n_bins"]):
        if g not in of_bin:
            assert got["status"][g] != 0 and got["best_contig"][g] == -1
            continue
        first, ng = min(of_bin[g]), len(of_bin[g])
        kg = run_of[first]
        uh = first - runs[kg][0]
        assert (got["status"][g], got["contig"][g], got["offset"][g], got["n_positions"][g]) == (0, kg, uh, ng)
        ent = {}  # contig -> [(reduced offset, count)]
        for p, v in rows.get(g, {}).items():
            k = run_of[p]
            x = p - runs[k][0] - (ng if k == kg and p > first else 0)
            ent.setdefault(k, []).append((x, v))

        def site(k, u):
            n_red = runs[k][1] - (ng if k == kg else 0)
            lo, hi = max(0, u - w), min(n_red, u + w)
            left = sum(v for x, v in ent.get(k, ()) if lo <= x < u)
            right = sum(v for x, v in ent.get(k, ()) if u <= x < hi)
            return left, right, hi - lo

        if runs[kg][1] - ng > 0:
            left, right, hosts = site(kg, uh)
            assert (got["home_hosts"][g], got["home_left"][g], got["home_right"][g]) == (hosts, left, right), g
        picked = []
        for which in ("best", "second"):
            top = None
            for k in sorted(ent):  # (a site with obs > 0 lies in a contig the row has an entry in)
                n_red = runs[k][1] - (ng if k == kg else 0)
                for u in range(0, n_red + 1) if not (k == kg and n_red == 0) else ():
                    left, right, hosts = site(k, u)
                    if hosts < mh or left + right == 0 or (k == kg and abs(u - uh) < 2 * w):
                        continue
                    if picked and k == picked[0][2] and abs(u - picked[0][3]) < 2 * w:
                        continue
                    x = (left + right, hosts, k, u, left, right)
                    if _better(x, top):
                        top = x
            if top is None:
                assert got[which + "_contig"][g] == -1
                break
            assert (got[which + "_contig"][g], got[which + "_offset"][g], got[which + "_hosts"][g], got[which + "_left"][g], got[which + "_right"][g]) == (
                top[2], top[3], top[1], top[4], top[5]), (g, which)
            picked.append(top)
        moved += bool(picked)
    assert moved > 20 and int(got["best_left"].max()) + int(got["best_right"].max()) > 2 ** 31


# ---- the check in front of upload_contacts


def test_as_int32_exact():
    from instagraal_amd.hip_lib import as_int32_exact

    ok = as_int32_exact(np.array([0, 5, 2 ** 31 - 1, -2 ** 31], np.int64), "cnt")
    assert ok.dtype == np.int32 and ok.flags.c_contiguous and ok.tolist() == [0, 5, 2 ** 31 - 1, -2 ** 31]
    same = np.arange(5, dtype=np.int32)
    assert as_int32_exact(same) is same or np.shares_memory(as_int32_exact(same), same)
    assert as_int32_exact(np.arange(10, dtype=np.int32)[::2]).flags.c_contiguous
    assert as_int32_exact(np.array([3.0, 2.0 ** 31 - 1]), "cnt").tolist() == [3, 2 ** 31 - 1]  # (whole floats pass)
    assert as_int32_exact([1, 2, 3]).tolist() == [1, 2, 3] and as_int32_exact(np.array([7], np.uint8)).tolist() == [7]
    assert as_int32_exact(np.zeros(0)).size == 0
    for bad in (np.array([1, 2 ** 31], np.int64), np.array([-2 ** 31 - 1], np.int64), np.array([2 ** 32 + 5], np.uint64), np.array([2 ** 31], np.uint32),
                np.array([1.5]), np.array([2.0 ** 31]), np.array([np.nan]), np.array([np.inf]), np.array([-2.0 ** 31 - 1]), np.array(["7"]),
                np.array([1 + 2j])):
        with pytest.raises(ValueError, match="cnt"):
            as_int32_exact(bad, "cnt")
    with pytest.raises(ValueError, match=r"1 of 2 values do not fit int32 \(the first: 2147483648 at index 1\)"):
        as_int32_exact(np.array([1, 2 ** 31], np.int64), "cnt")
    assert np.ascontiguousarray(np.array([2 ** 31], np.int64), np.int32)[0] == -2 ** 31  # what the conversion alone did
