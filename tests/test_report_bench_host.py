"""The kit the benches of the reports share (tools/_report_bench.py), driven with fake timed callables: no GPU library is loaded."""
import importlib.util
import json
import os

import numpy as np
import pytest

from conftest import ROOT

_spec = importlib.util.spec_from_file_location("_report_bench", os.path.join(ROOT, "tools", "_report_bench.py"))
kit = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kit)


class Fake:
    """a form of a pass: records its calls into a shared log; sample i of call c is 100 c + i, so a kept warm-up shows"""

    def __init__(self, name, log, checksums=None):
        self.name, self.log, self.checksums, self.calls = name, log, checksums, 0

    def __call__(self, n):
        self.log.append((self.name, n))
        ms = 100.0 * self.calls + np.arange(n, dtype=np.float32)
        ck = self.checksums[self.calls] if self.checksums else 7
        self.calls += 1
        return ms, ck


def test_alternate_calls_the_forms_in_turn_and_drops_each_blocks_warm_ups():
    log = []
    a, b = kit.alternate(Fake("a", log), Fake("b", log), reps=10, warmup=2)  # four blocks of 2 + ceil(10 / 4) = 5
    assert log == [("a", 5), ("b", 5)] * 4
    want = np.concatenate([100.0 * c + np.arange(2, 5) for c in range(4)])
    assert np.array_equal(a, want) and np.array_equal(b, want)
    log.clear()
    a, b = kit.alternate(Fake("a", log), Fake("b", log), reps=3, warmup=0, blocks=2)
    assert log == [("a", 2), ("b", 2)] * 2 and a.size == 4 and b.size == 4
    # rows of several passes per repetition: the blocks are stacked
    a, _ = kit.alternate(lambda n: (np.ones((n, 3), np.float32), 1), lambda n: (np.zeros((n, 3), np.float32), 1), reps=8, warmup=1)
    assert a.shape == (8, 3)


def test_alternate_raises_on_a_checksum_mismatch_in_any_block():
    for bad_block in range(4):
        log = []
        sums = [7] * 4
        sums[bad_block] = 8
        with pytest.raises(AssertionError, match="the two forms disagree"):
            kit.alternate(Fake("a", log), Fake("b", log, sums), reps=4, warmup=1)
        assert len(log) == 2 * (bad_block + 1)  # nothing runs behind the block that disagreed


def test_alternate_blocks_takes_any_number_of_forms_and_keeps_the_blocks_apart():
    log = []
    by = kit.alternate_blocks([Fake(k, log) for k in "abc"], reps=5, warmup=3, blocks=2)
    assert log == [("a", 6), ("b", 6), ("c", 6)] * 2
    assert [len(blocks) for blocks in by] == [2, 2, 2] and np.array_equal(by[2][1], 100.0 + np.arange(3, 6))
    with pytest.raises(AssertionError, match="scan"):
        kit.alternate_blocks([Fake("a", log), Fake("b", log), Fake("c", log, [7, 9])], reps=2, warmup=0, blocks=2, disagree="the forms of the scan disagree")


def test_put_times_rounds_and_names_as_the_tools_did():
    ms = np.array([0.0123456, 0.0100004, 0.0300049, 0.0200051], np.float64)  # median: (0.0123456 + 0.0200051) / 2 = 0.01617535
    out = dict(first=1)
    kit.put_times(out, "observed_combined_us", ms)
    assert list(out.items()) == [("first", 1), ("observed_combined_us", 16.18), ("observed_combined_min_us", 10.0)]
    out = {}
    kit.put_times(out, "tiles_plain_ms", ms)
    assert list(out.items()) == [("tiles_plain_ms", 0.0162), ("tiles_plain_min_ms", 0.01)]
    with pytest.raises(KeyError):
        kit.put_times(out, "seconds", ms)


def test_host_clock_runs_the_warm_ups_and_the_repetitions():
    calls = []
    ms = kit.host_clock_ms(lambda: calls.append(1), reps=5, warmup=2)
    assert len(calls) == 7 and ms >= 0.0 and ms == round(ms, 2)
    assert kit.host_clock_ms(lambda: calls.append(1), reps=2, warmup=0) >= 0.0 and len(calls) == 9


def test_shipped_flag_reads_the_define_and_fails_loudly_without_it(tmp_path):
    inc = tmp_path / "ig_host_some.inc"
    for value in (0, 1, 16):
        inc.write_text("/* which form ships */\n#define SOME_SHIP_COMBINE %d\n#define SOME_SHIP_COMBINED 5\n" % value)
        assert kit.shipped_flag(str(inc), "SOME_SHIP_COMBINE") == value
    with pytest.raises(ValueError, match="OTHER_SHIP_COMBINE"):
        kit.shipped_flag(str(inc), "OTHER_SHIP_COMBINE")
    assert kit.shipped_flag("ig_host_orient.inc", "ORIENT_SHIP_COMBINE") in (0, 1)  # (a name alone: csrc/ of the repository)


def test_ship_verdict_and_write_doc(tmp_path, capsys):
    for ok, built, shipped, asked in ((True, True, "combined", True), (False, True, "combined", False), (False, False, "one_atomic_per_end", True)):
        doc = dict(results=[])
        kit.ship_verdict(doc, ok, built)
        assert list(doc.items()) == [("results", []), ("combined_not_above_yardstick_everywhere", ok), ("observed_pass_shipped", shipped),
                                     ("shipped_form_is_what_the_figures_ask_for", asked)]
    out = tmp_path / "deeper" / "doc.json"
    kit.write_doc(doc, str(out))
    assert json.load(open(out)) == doc and json.loads(capsys.readouterr().out) == doc
    kit.write_doc(doc, str(out), show=doc["results"])
    assert json.loads(capsys.readouterr().out) == [] and open(out).read() == json.dumps(doc, indent=1)
