"""The rule of the combining idiom of the passes over the contacts (wave_runs / wave_run_sum, ig_kernels_wave.cuh: a run of a wave's
lanes with an equal key is summed inside the wave and issues one atomic) in a few lines of numpy, the inputs the direct GPU test
(test_hip_wave_runs.py) drives it with, and, here, without a GPU: the rule against a pure-Python brute force, and every property of
the inputs that the GPU test depends on, so that a generator cannot quietly stop producing the hard case."""
import ctypes as C
import os

import numpy as np
import pytest

WAVE, GROUP = 64, 256  # lanes of a wave, threads of a workgroup
GRID = 64              # DEBUG_WAVE_BLOCKS (ig_host_debug.inc): the workgroups of a launch at the most


# ---------------------------------------------------------------- the rule

def run_heads(keys):
    """head[k]: entry k opens a run -- the first lane of its wave, or a key other than the one in front"""
    keys = np.asarray(keys, np.int64)
    head = np.arange(keys.size) % WAVE == 0
    head[1:] |= keys[1:] != keys[:-1]
    return head


def wave_rule(keys, values, n_dest):
    """entry k adds values[k] to out[keys[k]] (a negative key: no entry) -> (out int64 [n_dest], the atomics: the maximal runs of
    equal keys inside aligned chunks of 64 whose key is >= 0 and whose sum is not 0)"""
    keys, values = np.asarray(keys, np.int64), np.asarray(values, np.int64)
    out = np.zeros(n_dest, np.int64)
    np.add.at(out, keys[keys >= 0], values[keys >= 0])
    first = np.nonzero(run_heads(keys))[0]
    sums = np.add.reduceat(values, first) if first.size else np.zeros(0, np.int64)
    return out, int(((keys[first] >= 0) & (sums != 0)).sum())


def brute_force(keys, values, n_dest):
    out, atomics = [0] * n_dest, 0
    for base in range(0, len(keys), WAVE):
        k = base
        while k < min(base + WAVE, len(keys)):
            end, total = k, 0
            while end < min(base + WAVE, len(keys)) and keys[end] == keys[k]:
                total += int(values[end])
                end += 1
            if keys[k] >= 0 and total != 0:
                out[int(keys[k])] += total
                atomics += 1
            k = end
    return np.array(out, np.int64).reshape(n_dest), atomics


# ---------------------------------------------------------------- the inputs: name -> (keys, values, n_dest, the forms: wide = 0 / 1)

RAGGED_N = (1, 63, 64, 65, 129)
BOUNDARY_ATOMICS = 11  # of the case "boundaries", counted by hand below
BIG_N = 100_000


def _ragged(n):
    return (np.arange(n) // 5) % 4, np.arange(n) - 7, 4, (0, 1)


def _skip():
    keys = np.concatenate([np.arange(WAVE), WAVE + np.arange(WAVE) // 8])  # a wave of heads only, then a wave of eight runs
    return keys, np.full(keys.size, 3), WAVE + 8, (0, 1)


def _boundaries():
    keys = np.full(9 * WAVE, -1)
    keys[40:84] = 1      # across a wave's end: two atomics
    keys[250:262] = 2    # across a workgroup's end (thread 255 -> 256): two
    keys[306:320] = 3    # ends at lane 63: one
    keys[320:325] = 4    # ... and what follows is its own run: one
    keys[383:390] = 5    # starts at lane 63: lane 63 alone, then the rest: two
    keys[512:576] = 6    # a whole wave of one key ...
    keys[520] = keys[530] = keys[531] = keys[532] = -1  # ... that lanes without a key split into three; wave 7 has no key at all
    return keys, np.arange(keys.size) % 11 + 1, 7, (0, 1)


def _big():
    rng = np.random.default_rng(7)
    lengths = rng.geometric(0.1, BIG_N)  # (more than enough runs)
    run_keys = np.where(rng.random(lengths.size) < 0.05, -1, rng.integers(0, 4000, lengths.size))
    return np.repeat(run_keys, lengths)[:BIG_N], rng.integers(-1000, 1001, BIG_N), 4000, (0, 1)


CASES = {"ragged_%d" % n: _ragged(n) for n in RAGGED_N}
CASES.update(
    equal=(np.full(WAVE, 2), np.arange(1, WAVE + 1), 3, (0, 1)),
    skip=_skip(),
    boundaries=_boundaries(),
    cancel=(np.repeat([0, 1, 2], [4, 4, 2]), np.array([3, -3, 5, -5, 1, 2, 3, 4, -7, 7]), 3, (0, 1)),
    negative=(np.zeros(10, int), -np.arange(1, 11), 1, (0, 1)),
    narrow_max=(np.zeros(WAVE, int), np.full(WAVE, 2**25 - 1), 1, (0, 1)),
    wide_max=(np.zeros(WAVE, int), np.full(WAVE, 2**31 - 1), 1, (1,)),
    big=_big(),
)

_WANT = {}


def want(name):
    """the rule's result, computed once per input and shared"""
    if name not in _WANT:
        keys, values, n_dest, _ = CASES[name]
        _WANT[name] = wave_rule(keys, values, n_dest)
    return _WANT[name]


# ---------------------------------------------------------------- without a GPU

@pytest.mark.parametrize("name", sorted(CASES))
def test_the_rule_equals_the_brute_force(name):
    keys, values, n_dest, _ = CASES[name]
    out, atomics = want(name)
    b_out, b_atomics = brute_force(keys, values, n_dest)
    assert out.tobytes() == b_out.tobytes() and atomics == b_atomics


def _runs(keys):
    """(first, behind) of every run"""
    first = np.nonzero(run_heads(keys))[0]
    return first, np.append(first[1:], len(keys))


def test_the_inputs_hold_the_cases_the_gpu_test_is_there_for():
    for name, (keys, values, n_dest, wides) in CASES.items():
        assert keys.shape == values.shape and keys.max() < n_dest and keys.min() >= -1, name
        first, behind = _runs(keys)
        sums = np.add.reduceat(np.asarray(values, np.int64), first)
        if 0 in wides:  # the 32-bit form: no value and no run's sum beyond an int
            assert np.abs(values).max() < 2**31 and np.abs(sums).max() < 2**31, name
    assert [CASES["ragged_%d" % n][0].size for n in RAGGED_N] == [1, 63, 64, 65, 129]  # a ragged last wave on either side of a full one
    assert (CASES["ragged_129"][1] < 0).any() and (CASES["ragged_129"][1] == 0).any()
    assert len(set(CASES["equal"][0])) == 1 and want("equal")[1] == 1 and want("equal")[0][2] == WAVE * (WAVE + 1) // 2
    heads = run_heads(CASES["skip"][0])
    assert heads[:WAVE].all() and not heads[WAVE:].all() and want("skip")[1] == WAVE + 8  # the skip path next to a wave with runs

    keys = CASES["boundaries"][0]
    first, behind = _runs(keys)
    runs = {(int(keys[f]), int(f), int(b)) for f, b in zip(first, behind)}
    assert {(1, 40, 64), (1, 64, 84)} <= runs                                    # a run across a wave's end
    assert {(2, 250, 256), (2, 256, 262)} <= runs and 256 % GROUP == 0           # ... and across a workgroup's
    assert (3, 306, 320) in runs and 320 % WAVE == 0 and (4, 320, 325) in runs   # a run that ends at lane 63
    assert (5, 383, 384) in runs and 383 % WAVE == 63 and (5, 384, 390) in runs  # one that starts there
    assert {(6, 512, 520), (6, 521, 530), (6, 533, 576)} <= runs                 # lanes without a key inside a run split it
    assert (keys[448:512] == -1).all() and (-1, 448, 512) in runs               # a whole wave without a key
    assert want("boundaries")[1] == BOUNDARY_ATOMICS == sum(1 for k, _, _ in runs if k >= 0)

    out, atomics = want("cancel")
    assert out.tolist() == [0, 10, 0] and atomics == 1  # runs whose values cancel issue nothing
    assert want("negative")[1] == 1 and want("negative")[0][0] == -55
    assert want("narrow_max")[0][0] == WAVE * (2**25 - 1) < 2**31
    assert want("wide_max")[0][0] == WAVE * (2**31 - 1) > 2**32 and CASES["wide_max"][3] == (1,)

    keys, values, n_dest, _ = CASES["big"]
    first, behind = _runs(keys)
    assert keys.size == BIG_N > GRID * GROUP  # more than one pass of the grid-stride loop
    assert (keys == -1).any() and (behind - first).max() > 32 and np.median(behind - first) < 10 and want("big")[1] > BIG_N // 20


def test_the_debug_symbol_exists_in_the_built_library():
    from instagraal_amd import hip_lib

    if not os.path.exists(hip_lib.LIB_PATH):
        pytest.fail("libinstagraal_hip.so is not built: run __graft_entry__.build()")
    assert hasattr(C.CDLL(hip_lib.LIB_PATH), "ig_debug_wave_runs")
    header = open(os.path.join(hip_lib.ROOT, "include", "instagraal_hip.h")).read()
    assert ("int ig_debug_wave_runs(ig_ctx* ctx, const int32_t* keys, const int64_t* values, int64_t n, int32_t n_dest, int32_t wide, int64_t* out, "
            "int64_t* atomics);") in header
    assert callable(hip_lib.Context.debug_wave_runs)
    assert any(d.endswith("ig_kernels_wave.cuh") for d in hip_lib.DEPS)  # a change of the header rebuilds the library
    source = open(os.path.join(hip_lib.HERE, "csrc", "ig_host_debug.inc")).read()
    assert "#define DEBUG_WAVE_BLOCKS %d\n" % GRID in source
