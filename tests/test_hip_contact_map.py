"""GPU tests of the contact map of the current genome (ig_contact_map_order / ig_contact_map, sampler.contact_map,
sampler.display_current_matrix) against what the reference's own ``display_current_matrix`` (CL:2555-2606) produced on two ``tiny``
trajectories (tests/golden/matrix_tiny_*.npz, tools/gen_golden_matrix.py), and against a host restatement at the headline shape."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FIXTURES = ("matrix_tiny_plain", "matrix_tiny_bomb")


def _sampler(cfg, seed=None, coo=False):
    from instagraal_amd import synth
    from instagraal_amd.sampler import sampler as hip_sampler

    prob = synth.make_problem(*synth.CONFIGS[cfg])
    if seed is not None:
        np.random.seed(seed)
    extra = dict(coo=(prob.coo_row, prob.coo_col, prob.coo_cnt)) if coo else {}
    s = hip_sampler(**prob.sampler_kwargs(), device_id=0, **extra)
    s.set_param_simu(dict(prob.params))
    s.bins = np.arange(1.0, 60.0, 1.0)
    s.eval_likelihood_init()
    return prob, s


def _dict_of(g):
    ends = np.cumsum(g["dict_lengths"])
    return {int(k): g["dict_values"][e - n:e].tolist() for k, n, e in zip(g["dict_keys"], g["dict_lengths"], ends)}


def _block_sums(full, b):
    """the T x T matrix under the binning rule: pixel of position r = r // b"""
    T = full.shape[0]
    side = -(-T // b)
    pad = np.zeros((side * b, side * b), np.int64)
    pad[:T, :T] = full
    return pad.reshape(side, b, side, b).sum(axis=(1, 3))


@pytest.mark.parametrize("name", FIXTURES)
def test_map_of_the_fixture_state_is_the_reference_matrix(name, tmp_path):
    from instagraal_amd import contact_map as cmap

    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    prob, s = _sampler(str(g["config"]))
    s.ctx.upload_state(g["state"])
    want = g["matrix"].astype(np.int64)
    T = want.shape[0]
    assert np.array_equal(s.ctx.contact_map_order(), g["full_order_high"])
    img, b = s.contact_map(max_side=T)
    assert b == 1 and img.dtype == np.int64 and np.array_equal(img, want)
    img, b = s.contact_map(max_side=T + 1000)
    assert b == 1 and np.array_equal(img, want)
    for max_side in (T - 1, 100, 7, 1):
        img, b = s.contact_map(max_side=max_side)
        assert (b, img.shape[0]) == cmap.binning(T, max_side) and img.shape[0] <= max_side
        assert np.array_equal(img, _block_sums(want, b)), max_side
    assert np.array_equal(s.contact_map()[0], want)  # the default max_side is beyond T here
    png = str(tmp_path / "m.png")
    full_order, dict_contig, full_order_high = s.display_current_matrix(png)
    assert full_order == g["full_order"].tolist() and full_order_high == g["full_order_high"].tolist()
    assert {int(k): v for k, v in dict_contig.items()} == _dict_of(g)
    assert open(png, "rb").read(8) == b"\x89PNG\r\n\x1a\n" and os.path.getsize(png) > 1000
    assert float(np.percentile(s.contact_map(T)[0], 99)) == float(g["vmax"])  # what the picture's colour scale is cut at
    s.free_gpu()


@pytest.mark.parametrize("name", FIXTURES)
def test_map_after_committed_batch_moves(name):
    """the fixture's state reached by replaying its moves through step_sampler_batch from the seed: the tables the pass reads are
    current behind moves committed in batches on the device"""
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    prob, s = _sampler(str(g["config"]), seed=int(g["seed"]))
    if bool(g["bomb"]):
        s.bomb_the_genome()
    frags = np.arange(0, s.n_new_frags)
    np.random.shuffle(frags)
    assert np.array_equal(frags[:int(g["n_moves"])], g["frag"])
    s.step_sampler_batch(frags[:int(g["n_moves"])], 5)
    assert np.array_equal(s.ctx.contact_map_order(), g["full_order_high"])
    img, b = s.contact_map(max_side=g["matrix"].shape[0])
    assert b == 1 and np.array_equal(img, g["matrix"])
    assert np.array_equal(s.gpu_vect_frags.copy_from_gpu().soa17(), g["state"])
    s.free_gpu()


def test_the_pass_disturbs_nothing():
    outs = []
    for with_map in (False, True):
        prob, s = _sampler("small", seed=3)
        frags = np.random.permutation(prob.n_frags)[:200]
        res = [s.step_sampler_batch(frags[:100], 5)]
        if with_map:
            img, _ = s.contact_map(max_side=256)
            order = s.ctx.contact_map_order()
            assert img.sum() > 0 and order.size == prob.n_sub_frags
        res.append(s.step_sampler_batch(frags[100:], 5))
        sums, ints = s.ctx.debug_globals()
        _, _, limbs = s.ctx.full_likelihood(0)
        assert [int(x) for x in sums[:5]] == [int(x) for x in limbs[:5]]
        outs.append((np.concatenate(res).tobytes(), s.gpu_vect_frags.copy_from_gpu().soa17(), sums.tolist(), ints.tolist(),
                     np.random.get_state()[1].copy(), np.random.get_state()[2], [int(x) for x in s.ctx.valid_insert()]))
        s.free_gpu()
    a, b = outs
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3]
    assert np.array_equal(a[4], b[4]) and a[5] == b[5] and a[6] == b[6]


def _host_map(state, prob, max_side):
    """restatement on the host: the order from the downloaded state, the contacts through np.bincount, symmetrised"""
    from instagraal_amd.hip_lib import FRAG_FIELDS

    col = {k: state[i].astype(np.int64) for i, k in enumerate(FRAG_FIELDS)}
    assert np.all(col["activ"] == 1)
    sub_len = col["sub_len"]
    first_sub = np.cumsum(sub_len) - sub_len  # the sub-fragments of a bin are consecutive in the table
    by = np.lexsort((col["pos"], col["id_c"]))  # the bins: contig by contig in ascending id, each in genome order
    w = sub_len[by]
    start = np.cumsum(w) - w
    bin_of = np.repeat(np.arange(by.size), w)
    j = np.arange(int(w.sum())) - start[bin_of]
    order = first_sub[by][bin_of] + np.where(col["ori"][by][bin_of] == -1, w[bin_of] - 1 - j, j)
    T = order.size
    where = np.full(prob.n_sub_frags, -1, np.int64)
    where[order] = np.arange(T)
    b = max(1, -(-T // max_side))
    side = -(-T // b)
    pi, pj = where[prob.coo_row] // b, where[prob.coo_col] // b
    ok = (where[prob.coo_row] >= 0) & (where[prob.coo_col] >= 0)
    upper = np.bincount(pi[ok] * side + pj[ok], weights=prob.coo_cnt[ok].astype(np.float64), minlength=side * side)
    assert upper.max() < 2.0 ** 52  # (the float sums of integers are exact)
    upper = upper.astype(np.int64).reshape(side, side)
    return upper + upper.T, b, order, int(prob.coo_cnt[ok].astype(np.int64).sum())


@pytest.mark.slow
def test_headline_shape_against_the_host_restatement():
    """cfg3 (50 k bins, 149 k sub-fragments, 50 M contacts) after 2 000 batch moves, 2048 pixels a side"""
    prob, s = _sampler("cfg3", coo=True)
    np.random.seed(4)
    frags = np.random.permutation(prob.n_frags)[:2000].astype(np.int32)
    s.step_sampler_batch(frags, 5)
    img, b = s.contact_map(max_side=2048)
    state = s.gpu_vect_frags.copy_from_gpu().soa17()
    want, wb, order, placed_counts = _host_map(state, prob, 2048)
    assert np.array_equal(s.ctx.contact_map_order(), order)
    assert b == wb and img.shape == want.shape and img.shape[0] <= 2048
    assert np.array_equal(img, want)
    assert np.array_equal(img, img.T)
    assert int(img.sum()) == 2 * placed_counts  # (+ the diagonal term: a sampler built from coo= has none)
    assert np.array_equal(s.contact_map(max_side=2048)[0], img)  # the same from run to run
    ms_a, sum_a = s.ctx.debug_contact_map_time(2048, combine=True, n=2)
    ms_b, sum_b = s.ctx.debug_contact_map_time(2048, combine=False, n=2)
    print("contact map pass at cfg3, 2048 px: combined %.1f us, one atomic per contact end %.1f us" % (1e3 * ms_a.min(), 1e3 * ms_b.min()))
    assert sum_a == sum_b == int(img.sum())
    s.free_gpu()


def test_errors_are_loud():
    from instagraal_amd import hip_lib
    from instagraal_amd.sampler import PARAM_NAMES

    prob, s = _sampler("tiny")
    for bad in (0, -5):
        with pytest.raises(hip_lib.HipError):
            s.contact_map(max_side=bad)
        side, b = C.c_int32(), C.c_int32()
        buf = np.full(16, -7, np.int64)
        rc = hip_lib.lib().ig_contact_map(s.ctx._h, C.c_int32(bad), C.c_void_p(buf.ctypes.data), C.c_int64(buf.size), C.byref(side), C.byref(b))
        assert rc != 0 and b"max_side" in hip_lib.lib().ig_last_error() and np.all(buf == -7)
    # a buffer that is too short: an error, not a truncated image
    T = prob.n_sub_frags
    buf = np.full(64 * 64 + 8, -7, np.int64)
    side, b = C.c_int32(), C.c_int32()
    rc = hip_lib.lib().ig_contact_map(s.ctx._h, C.c_int32(64), C.c_void_p(buf.ctypes.data), C.c_int64(64 * 64 - 1), C.byref(side), C.byref(b))
    assert rc != 0 and b"buffer" in hip_lib.lib().ig_last_error()
    assert np.all(buf == -7)  # nothing written, within the capacity or past it
    assert side.value == 64 and b.value == -(-T // 64)  # ... but the caller learns the size it needs
    rc = hip_lib.lib().ig_contact_map(s.ctx._h, C.c_int32(64), C.c_void_p(buf.ctypes.data), C.c_int64(64 * 64), C.byref(side), C.byref(b))
    assert rc == 0 and np.all(buf[64 * 64:] == -7) and buf[:64 * 64].sum() == 2 * int(prob.coo_cnt.astype(np.int64).sum())
    # between ig_nuis_begin and ig_nuis_end the calls refuse, and the step ends as if nothing had happened
    cands = s.return_neighbours(3, 5)
    p8 = np.array([float(s.param_simu[k][0]) for k in PARAM_NAMES], np.float32)
    s.ctx.nuis_begin(3, sorted(int(x) for x in cands if x != 3), p8, s.mean_kb())
    with pytest.raises(hip_lib.HipError, match="in flight"):
        s.ctx.contact_map(64)
    with pytest.raises(hip_lib.HipError, match="in flight"):
        s.ctx.contact_map_order()
    s.ctx.nuis_end()
    assert s.contact_map(64)[0].shape == (64, 64)
    s.free_gpu()


def test_run_instagraal_save_matrix_writes_one_picture_per_cycle(tmp_path):
    from instagraal_amd import synth
    from instagraal_amd.simulation import run_instagraal

    data, out = str(tmp_path / "data"), str(tmp_path / "out")
    synth.write_text_dataset(data, n_contigs=10, mean_frags=110, seed=7, contacts_per_frag=40)
    np.random.seed(17)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        p2 = run_instagraal(data, os.path.join(data, "genome.fa"), output_folder=out, level=2, cycles=2, bomb=True, save_matrix=True)
    # (no "ignored" warning any more, and no picture that could not be written)
    assert not [str(w.message) for w in caught if "save_matrix" in str(w.message) or "could not write the matrix" in str(w.message)]
    folder = p2.simulation.output_folder
    for j in range(2):
        assert open(os.path.join(folder, "matrix_cycle_%d.png" % j), "rb").read(8) == b"\x89PNG\r\n\x1a\n"
    assert not os.path.exists(os.path.join(folder, "matrix_cycle_2.png"))
    # real input: the matrix has a diagonal (self-contacts), which the host adds -- the reference's matrix entry for entry
    s = p2.simulation.sampler
    T = int(s.n_new_sub_frags)
    full_order, dict_contig, order = s.display_current_matrix(str(tmp_path / "again.png"), max_side=T)
    assert sorted(order) == list(range(T)) and sorted(full_order) == list(range(int(s.n_new_frags)))
    dense = s.sparse_matrix.toarray()
    img, b = s.contact_map(max_side=T)
    assert b == 1 and np.array_equal(img, dense[np.ix_(order, order)])
    p2.simulation.release()
