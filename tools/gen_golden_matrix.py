#!/usr/bin/env python3
"""Generate tests/golden/matrix_*.npz by running the REFERENCE's own ``sampler.display_current_matrix`` (CL:2555-2606).

Runs only in the authoring container (needs the reference checkout), like tools/gen_golden.py: the reference's
``instagraal.cuda_lib_gl_single.sampler`` is imported unmodified over the functional fake ``pycuda`` in tools/fake_pycuda (kernels:
oracle/ig_oracle_*.c, deterministic arithmetic), set up and moved exactly as gen_golden.py's cases are; then its own
``display_current_matrix`` runs on a temporary file.  What it returns -- ``full_order``, ``dict_contig``, ``full_order_high`` -- and
what it hands to ``Axes.imshow`` -- the matrix and ``vmax`` -- are stored with the 17 x N state they belong to.

Only numeric arrays are stored (no picture, no reference source).

usage:  python tools/gen_golden_matrix.py [--out tests/golden] [--check]
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tools", "fake_pycuda"))
sys.path.insert(0, ROOT)
sys.path.insert(1, "/root/reference/src")

CASES = {
    # name: (config, seed, n_moves, bomb)
    "matrix_tiny_plain": ("tiny", 11, 40, False),
    "matrix_tiny_bomb": ("tiny", 12, 40, True),
}


def run_case(name, outdir):
    import matplotlib

    matplotlib.use("Agg")
    from matplotlib.axes import Axes

    from instagraal_amd import synth
    from oracle import oracle_lib as ol
    import pycuda.driver as cuda
    from instagraal.cuda_lib_gl_single import sampler as ref_sampler

    cfg, seed, n_moves, bomb = CASES[name]
    ol.set_mode(ol.MODE_DET)
    prob = synth.make_problem(*synth.CONFIGS[cfg])
    kw = prob.sampler_kwargs()
    np.random.seed(seed)
    s = ref_sampler(*[kw[k] for k in kw])
    # what estimate_parameters_rippe does after the fit (CL:2343-2349), with fixed parameters: as tools/gen_golden.py
    p = prob.params
    par = np.array([(p["kuhn"], p["lm"], p["c1"], p["slope"], p["d"], p["d_max"], p["fact"], p["v_inter"])], dtype=s.param_simu_rippe)
    s.param_simu = par
    s.param_simu_test = s.param_simu
    s.gpu_param_simu = cuda.mem_alloc(s.param_simu.nbytes)
    s.gpu_param_simu_test = cuda.mem_alloc(s.param_simu.nbytes)
    cuda.memcpy_htod(s.gpu_param_simu, s.param_simu)
    cuda.memcpy_htod(s.gpu_param_simu_test, s.param_simu_test)
    s.bins = np.arange(1.0, 60.0, 1.0)
    s.eval_likelihood_init()
    if bomb:
        s.bomb_the_genome()
    list_frags = np.arange(0, s.n_new_frags)
    np.random.shuffle(list_frags)  # IG:213
    for id_frag in list_frags[:n_moves]:
        s.step_sampler(id_frag, 5, s.dt)

    seen = {}
    imshow = Axes.imshow

    def capture(self, X, *a, **k):
        seen["matrix"] = np.array(X)
        seen["vmax"] = float(k["vmax"])
        return imshow(self, X, *a, **k)

    Axes.imshow = capture
    try:
        with tempfile.TemporaryDirectory() as tmp:
            png = os.path.join(tmp, "m.png")
            full_order, dict_contig, full_order_high = s.display_current_matrix(png)
            assert os.path.getsize(png) > 0
    finally:
        Axes.imshow = imshow
    matrix = seen["matrix"]
    assert np.array_equal(matrix, matrix.astype(np.int32)) and np.array_equal(matrix, matrix.T)
    g = s.gpu_vect_frags
    g.copy_from_gpu()
    state = np.stack([getattr(g, k) if k != "next" else g.next for k in ol.FRAG_FIELDS]).astype(np.int32)
    keys = sorted(dict_contig)
    out = os.path.join(outdir, name + ".npz")
    np.savez_compressed(
        out, config=cfg, seed=seed, bomb=bomb, n_moves=n_moves, frag=np.asarray(list_frags[:n_moves], np.int32), state=state,
        full_order=np.asarray(full_order, np.int32), full_order_high=np.asarray(full_order_high, np.int32),
        dict_keys=np.asarray(keys, np.int32), dict_lengths=np.asarray([len(dict_contig[k]) for k in keys], np.int32),
        dict_values=np.asarray([x for k in keys for x in dict_contig[k]], np.int32), matrix=matrix.astype(np.int32),
        vmax=np.float64(seen["vmax"]))
    print("wrote", out, "bins", state.shape[1], "contigs", len(keys), "sub-fragments", len(full_order_high), "reversed bins",
          int((state[13] == -1).sum()), "vmax", seen["vmax"])


def check(a):
    """regenerate into a temporary directory and compare with the committed files, array for array"""
    tmp = tempfile.mkdtemp(prefix="ig_golden_matrix_check_")
    subprocess.check_call([sys.executable, os.path.abspath(__file__), "--out", tmp], stdout=subprocess.DEVNULL)
    bad = n_arrays = 0
    for name in CASES:
        f = name + ".npz"
        ref_path = os.path.join(a.out, f)
        if not os.path.exists(ref_path):
            print("MISSING in %s: %s" % (a.out, f))
            bad += 1
            continue
        new, old = np.load(os.path.join(tmp, f), allow_pickle=False), np.load(ref_path, allow_pickle=False)
        if sorted(new.files) != sorted(old.files):
            print("KEYS differ in %s: %s" % (f, sorted(set(new.files) ^ set(old.files))))
            bad += 1
        for k in sorted(set(new.files) & set(old.files)):
            n_arrays += 1
            x, y = new[k], old[k]
            if not (x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y)):
                print("DIFFERS: %s:%s" % (f, k))
                bad += 1
    print("gen_golden_matrix --check: %d arrays compared, %d differences" % (n_arrays, bad))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--check", action="store_true",
                    help="regenerate into a temporary directory and compare with the committed files (--out), array for array")
    a = ap.parse_args()
    if a.check:
        sys.exit(check(a))
    os.makedirs(a.out, exist_ok=True)
    a.out = os.path.abspath(a.out)
    os.chdir(tempfile.mkdtemp())  # the reference's log.py drops a log file in the CWD
    for name in CASES:
        run_case(name, a.out)


if __name__ == "__main__":
    main()
