"""The host side of the BCD statistics that needs no device: the options of the two drivers, the stop rule, the bytes of
struct dflow_bcd_stats as a dict and the JSON file of the per-sweep history."""
import json
import os
import runpy
import struct

import pytest

from conftest import PKG, ROOT, pkg


def bcd_cli():
    return runpy.run_path(os.path.join(ROOT, PKG, "python bcd.py"), run_name="bcd_cli")


def test_python_bcd_options():
    ns = bcd_cli()
    B = pkg("bcdstats")
    ap = ns["parser"]()
    a = ap.parse_args(["6", "0", "4"])
    assert (a.picindex, a.backward, a.bcd_times) == ("6", "0", 4)
    assert a.bcd_stats is False and a.stop_changed is None and a.stop_energy is None
    assert B.stop_from_args(a) is None                                   # today's run: no statistics, no extra launch
    a = ap.parse_args(["6", "1", "12", "--stats"])
    assert a.bcd_stats is True and B.stop_from_args(a) == {}
    a = ap.parse_args(["6", "1", "12", "--stop-changed", "0.01", "--stop-energy", "1e-4"])
    assert B.stop_from_args(a) == {"changed_frac": 0.01, "rel_energy": 1e-4}
    a = ap.parse_args(["6", "1", "12", "--stop-energy", "0"])
    assert B.stop_from_args(a) == {"rel_energy": 0.0}
    with pytest.raises(SystemExit):
        ap.parse_args(["6", "1", "12", "--stop-changed", "few"])


def test_run_batch_options():
    B = pkg("bcdstats")
    ap = pkg("run_batch").parser()
    a = ap.parse_args([])
    assert a.bcd_stats is False and B.stop_from_args(a) is None
    a = ap.parse_args(["--bcd-stats"])
    assert a.bcd_stats is True and B.stop_from_args(a) == {}
    a = ap.parse_args(["--stop-changed", "0.005"])
    assert B.stop_from_args(a) == {"changed_frac": 0.005}
    a = ap.parse_args(["--bcd-stats", "--stop-energy", "0.001", "--bcd-times", "12"])
    assert B.stop_from_args(a) == {"rel_energy": 0.001} and a.bcd_times == 12


def test_check_stop():
    B = pkg("bcdstats")
    assert B.check_stop(None) is None and B.check_stop({}) == {}
    assert B.check_stop({"changed_frac": 1}) == {"changed_frac": 1.0}
    for bad in ({"changed": 0.1}, {"rel_energy": float("nan")}, 0.1, [("changed_frac", 0.1)]):
        with pytest.raises(ValueError):
            B.check_stop(bad)


def test_stats_dict_and_stop_rule():
    B = pkg("bcdstats")
    buf = struct.pack("<5Qd", 1000, 7, 3, 12, 0, 40.0)
    assert len(buf) == B.STATS_BYTES
    d = B.stats_dict(buf, 0.05, 48)
    assert d == dict(smooth_sum=1000, n_pairs_trunc=7, n_data_trunc=3, n_changed=12, n_bad_label=0, data_sum=40.0,
                     energy=0.05 * 40.0 + 1000.0, changed_frac=0.25)
    with pytest.raises(ValueError):
        B.stats_dict(buf[:40], 0.05, 48)
    # changed_frac: at most this fraction
    assert B.should_stop({"changed_frac": 0.25}, d, 2000.0) and not B.should_stop({"changed_frac": 0.24}, d, 2000.0)
    # rel_energy: E went 1010 -> 1002, a drop of 0.79 %
    assert B.should_stop({"rel_energy": 0.01}, d, 1010.0) and not B.should_stop({"rel_energy": 0.005}, d, 1010.0)
    # a rise of E stops the pass for every rel_energy >= 0, and never for a very negative one
    assert B.should_stop({"rel_energy": 0.0}, d, 1001.0) and not B.should_stop({"rel_energy": -1e9}, d, 1001.0)
    assert not B.should_stop({}, d, 1001.0)
    # E >= 0 by the contract of the data costs; a negative one is refused, not compared
    with pytest.raises(ValueError):
        B.should_stop({"rel_energy": 0.01}, d, -5.0)
    # either criterion is enough
    assert B.should_stop({"changed_frac": 0.0, "rel_energy": 0.01}, d, 1010.0)


def synthetic_history(n):
    B = pkg("bcdstats")
    hist = []
    for w in range(n + 1):
        d = B.stats_dict(struct.pack("<5Qd", 3000 - 100 * w, 50 - w, 9, 0 if w == 0 else 640 >> w, 0, 800.0 - w), 0.05, 64 * 48)
        d["sweep"] = w
        hist.append(d)
    return hist


def test_history_json_schema(tmp_path):
    B = pkg("bcdstats")
    h0, h1 = synthetic_history(3), synthetic_history(1)
    path = tmp_path / "bcd_stats.json"
    B.write_history_json(str(path), [("pair 0 backward=0", h0), ("pair 0 backward=1", h1)], 0.05, 4, {"changed_frac": 0.01}, (64, 48))
    doc = json.loads(path.read_text())
    assert set(doc) == {"size", "lamda", "bcd_times", "stop", "fields", "passes"}
    assert doc["size"] == [64, 48] and doc["lamda"] == 0.05 and doc["bcd_times"] == 4 and doc["stop"] == {"changed_frac": 0.01}
    assert doc["fields"] == ["sweep", "smooth_sum", "n_pairs_trunc", "n_data_trunc", "n_changed", "n_bad_label", "data_sum",
                             "energy", "changed_frac"]
    assert [p["pass"] for p in doc["passes"]] == ["pair 0 backward=0", "pair 0 backward=1"]
    assert [p["sweeps_run"] for p in doc["passes"]] == [3, 1]
    for p, h in zip(doc["passes"], (h0, h1)):
        assert len(p["history"]) == len(h)
        for row, want in zip(p["history"], h):
            assert list(row) == doc["fields"]
            assert row == {k: want[k] for k in doc["fields"]}
            assert row["energy"] == 0.05 * row["data_sum"] + row["smooth_sum"]
    # no stop rule: an empty object, not null
    assert B.history_json([("p", h1)], 0.05, 1, None, (64, 48))["stop"] == {}
    line = B.format_row(h0[2])
    assert line.split()[:4] == ["sweep", "2", "changed", "160"] and "smooth 2800" in line and " E " in line
