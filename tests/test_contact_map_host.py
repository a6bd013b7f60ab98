"""CPU tests of the contact map's host side (instagraal_amd.contact_map, tools/gen_golden_matrix.py) against what the reference's own
``sampler.display_current_matrix`` (CL:2555-2606) returned on the two ``tiny`` trajectories of tests/golden/matrix_tiny_*.npz."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FIXTURES = ("matrix_tiny_plain", "matrix_tiny_bomb")


def _dict_of(g):
    ends = np.cumsum(g["dict_lengths"])
    return {int(k): g["dict_values"][e - n:e].tolist() for k, n, e in zip(g["dict_keys"], g["dict_lengths"], ends)}


def _triple(state, prob):
    from instagraal_amd import contact_map as cmap
    from instagraal_amd.hip_lib import FRAG_FIELDS

    col = {k: state[i] for i, k in enumerate(FRAG_FIELDS)}
    return cmap.genome_order(col["pos"], col["id_c"], col["activ"], col["id_d"], col["ori"], prob.np_sub_frags_id)


@pytest.mark.parametrize("name", FIXTURES)
def test_genome_order_reproduces_the_reference(name):
    from instagraal_amd import synth

    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    prob = synth.make_problem(*synth.CONFIGS[str(g["config"])])
    full_order, dict_contig, full_order_high = _triple(g["state"], prob)
    assert full_order == g["full_order"].tolist()
    assert full_order_high == g["full_order_high"].tolist()
    assert {int(k): v for k, v in dict_contig.items()} == _dict_of(g)
    assert list(dict_contig) == sorted(dict_contig)  # the reference fills it in ascending id
    assert (g["state"][13] == -1).any() and sorted(full_order_high) == list(range(prob.n_sub_frags))  # both strands; everything placed


def test_a_contig_with_an_inactive_bin_is_left_out():
    from instagraal_amd import synth

    g = np.load(os.path.join(GOLDEN, "matrix_tiny_plain.npz"))
    prob = synth.make_problem(*synth.CONFIGS[str(g["config"])])
    state = g["state"].copy()
    ref = _dict_of(g)
    victim = next(k for k in sorted(ref) if len(ref[k]) > 1)  # a multi-bin contig
    bins_of = np.nonzero(state[2] == victim)[0]
    state[15, bins_of[1]] = 0  # one of its bins inactive
    full_order, dict_contig, full_order_high = _triple(state, prob)
    gone = set(ref[victim])
    assert dict_contig[victim] == [] and not gone & set(full_order)
    assert full_order == [f for f in g["full_order"].tolist() if f not in gone]
    sub_gone = {int(prob.np_sub_frags_id[k][f]) for f in gone for k in "xyz"[:int(prob.np_sub_frags_id["w"][f])]}
    assert full_order_high == [s for s in g["full_order_high"].tolist() if s not in sub_gone]
    for k in ref:
        if k != victim:
            assert dict_contig[k] == ref[k]


@pytest.mark.parametrize("T", [1, 7, 893, 150_001])
@pytest.mark.parametrize("max_side", [1, 64, 893, 2048])
def test_binning_rule(T, max_side):
    from instagraal_amd import contact_map as cmap

    b, side = cmap.binning(T, max_side)
    assert b == max(1, -(-T // max_side)) and side == -(-T // b)
    assert 1 <= side <= max_side
    px = cmap.pixel_of(np.arange(T), b)
    assert px[0] == 0 and px[-1] == side - 1  # the last pixel is not empty
    assert np.array_equal(px, np.arange(T) // b) and np.all(np.diff(px) >= 0) and np.bincount(px).max() == b
    if max_side >= T:
        assert (b, side) == (1, T)  # full resolution: one sub-fragment per pixel
    with pytest.raises(ValueError):
        cmap.binning(T, 0)


@pytest.mark.skipif(not os.path.isdir("/root/reference/src/instagraal"), reason="needs the reference checkout (authoring container only)")
def test_matrix_goldens_regenerate_from_the_reference():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_golden_matrix.py"), "--check"], capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "0 differences" in p.stdout


def test_import_leaves_matplotlib_alone():
    code = ("import sys; import instagraal_amd, instagraal_amd.sampler, instagraal_amd.simulation, instagraal_amd.contact_map; "
            "sys.exit(1 if any(m == 'matplotlib' or m.startswith('matplotlib.') for m in sys.modules) else 0)")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]


def test_fixture_matrix_is_the_symmetrised_input_under_the_order():
    """the fixture is self-consistent with the problem it came from: the captured matrix is (m + m.T)[order][:, order], vmax its 99th
    percentile -- what the GPU tests hold ig_contact_map to"""
    from instagraal_amd import synth

    for name in FIXTURES:
        g = np.load(os.path.join(GOLDEN, name + ".npz"))
        prob = synth.make_problem(*synth.CONFIGS[str(g["config"])])
        m = prob.sampler_kwargs()["sparse_matrix"]
        dense = (m + m.T).toarray()
        o = g["full_order_high"]
        assert np.array_equal(dense[np.ix_(o, o)], g["matrix"])
        assert float(np.percentile(g["matrix"], 99)) == float(g["vmax"])
