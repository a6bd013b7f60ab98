"""What the benches of the reports on the current genome (tools/*_bench.py) share: the sampler they measure on, the loop in which the
forms of a pass alternate, the rounding of the figures, the whole call on the host clock, the ship flag of the source the library is
built from, and the file they write.  A bench keeps its `measure`: which passes it times, in which order, under which keys.  Importing
this module loads no GPU library (tests/test_report_bench_host.py drives it with fake timed callables)."""
import json
import os
import re
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "instagraal_amd", "csrc")


def make_sampler(cfg, moves, prepare=None):
    """the synthetic problem `cfg` on device 0, built from coo=, parameters set, likelihood initialised; numpy seeded with 0, then
    prepare(sampler) if given, then `moves` batch moves -> (problem, sampler)"""
    from instagraal_amd import synth
    from instagraal_amd.sampler import sampler as hip_sampler

    prob = synth.make_problem(*synth.CONFIGS[cfg])
    s = hip_sampler(**prob.sampler_kwargs(), device_id=0, coo=(prob.coo_row, prob.coo_col, prob.coo_cnt))
    s.set_param_simu(dict(prob.params))
    s.eval_likelihood_init()
    np.random.seed(0)
    if prepare:
        prepare(s)
    if moves:
        s.step_sampler_batch(np.resize(np.random.permutation(prob.n_frags), moves).astype(np.int32), 5)
    return prob, s


def alternate_blocks(forms, reps, warmup, blocks=4, disagree="the forms disagree"):
    """The forms of one pass alternate in `blocks` blocks (other work shares the machine: a drift hits all alike).  Each form is a
    callable n -> (ms, checksum), ms with one row per repetition; it is called with warmup + ceil(reps / blocks) in every block, its
    warm-ups are dropped, and the checksums of a block must agree.  Per form, the list of its blocks' timed rows."""
    per = (reps + blocks - 1) // blocks
    by = [[] for _ in forms]
    for _ in range(blocks):
        sums = []
        for k, form in enumerate(forms):
            ms, ck = form(warmup + per)
            by[k].append(ms[warmup:])
            sums.append(ck)
        assert all(ck == sums[0] for ck in sums), disagree
    return by


def alternate(form_a, form_b, reps, warmup, blocks=4, disagree="the two forms disagree"):
    """alternate_blocks for two forms: their two concatenated sample arrays"""
    a, b = alternate_blocks((form_a, form_b), reps, warmup, blocks, disagree)
    return np.concatenate(a), np.concatenate(b)


def put_times(out, key, ms):
    """out[key], the median of the samples (milliseconds), and its `_min` twin: microseconds to 2 places under a key that ends in _us,
    milliseconds to 4 places under one that ends in _ms"""
    unit = key[-3:]
    scale, places = {"_us": (1e3, 2), "_ms": (1.0, 4)}[unit]
    out[key] = round(scale * float(np.median(ms)), places)
    out[key.replace(unit, "_min" + unit)] = round(scale * float(np.min(ms)), places)


def host_clock_ms(fn, reps, warmup):
    """the whole call on the host clock: the median of `reps` calls behind `warmup`, in milliseconds to 2 places"""
    t = []
    for _ in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return round(1e3 * float(np.median(t[warmup:])), 2)


def shipped_flag(inc_name, macro):
    """the integer `#define macro` has in csrc/inc_name (a path of its own is taken as it is): the source the library is built from"""
    src = open(os.path.join(CSRC, inc_name)).read()
    m = re.search(r"#define %s (\d+)" % re.escape(macro), src)
    if m is None:
        raise ValueError("%s: no #define %s <number>" % (inc_name, macro))
    return int(m.group(1))


def ship_verdict(doc, ok, built):
    """the three keys of a bench whose observed pass ships combined only if that form is nowhere above its yardstick"""
    doc["combined_not_above_yardstick_everywhere"] = ok
    doc["observed_pass_shipped"] = "combined" if built else "one_atomic_per_end"
    doc["shipped_form_is_what_the_figures_ask_for"] = built == ok


def write_doc(doc, out, show=None):
    """the document into `out` (its directory made), and it -- or `show` in its place -- on the standard output"""
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    json.dump(doc, open(out, "w"), indent=1)
    print(json.dumps(doc if show is None else show, indent=1))
