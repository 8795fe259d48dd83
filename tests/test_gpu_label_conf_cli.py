"""The command-line side of the label confidence on the GPU: "python bcd.py" --confidence writes the wrapper's margin plane, and
run_batch.py --confidence T carries every pass's margin to rank 0, gates the sparse field with it and evaluates the kind
"confident"; without the option both issue the calls they always issued and write the files they always wrote.  Run with
`pytest -m gpu`."""
import json
import os
import runpy

import numpy as np
import pytest

from call_log import BATCH_FLOWS, record_calls
from conftest import GOLDEN_NAMES, PKG, ROOT, pkg
from label_conf_ref import flow_gate_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def test_python_bcd_confidence_writes_the_wrappers_plane(torch_, golden, tmp_path, monkeypatch):
    pipeline, flowio = pkg("pipeline"), pkg("flowio")
    g = golden(GOLDEN_NAMES[0])
    H, W, ch, cw = (int(g[k]) for k in ("H", "W", "cellh", "cellw"))
    df = pipeline.DiscreteFlow(H, W, ch, cw, seed=int(g["seed"]))
    df.front_end(g["img1"], g["img2"])
    st = df.host_state()
    monkeypatch.chdir(tmp_path)
    for what, key in (("proposals_nakon_gausa", "proposals"), ("lcosts_nakon_gausa", "lcosts"), ("nprop", "nprop")):
        np.save(flowio.stage_name("01", "0", what), st[key])
    np.save(flowio.labels_name("01", "0", 0), st["bestlabels"])
    bcd = runpy.run_path(os.path.join(ROOT, PKG, "python bcd.py"), run_name="bcd_cli")
    names = record_calls(monkeypatch)
    bcd["main"](["1", "0", "2", "--cell", "%dx%d" % (ch, cw)])
    plain = list(names)
    assert "dflow_label_confidence" not in plain and not os.path.exists(flowio.margin_name("01", "0", 2))
    flow_plain = open(flowio.flow_name("01", "0", 2), "rb").read()
    del names[:]
    bcd["main"](["1", "0", "2", "--cell", "%dx%d" % (ch, cw), "--confidence", "--conf-mode", "data", "--conf-sep", "0"])
    assert names == plain + ["dflow_label_confidence"], "the option adds one call, after everything the run always issued"
    assert open(flowio.flow_name("01", "0", 2), "rb").read() == flow_plain
    got = np.load(flowio.margin_name("01", "0", 2))
    # the wrapper on the same state
    df.ceoBCD(2)
    want = df.confidence(mode="data", min_sep=0).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (H, W) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not np.array_equal(want, df.confidence().cpu().numpy()), "the options reach the call: the default plane is another one"


def test_run_batch_confidence(torch_, tmp_path, monkeypatch, capsys):
    flowio, rb = pkg("flowio"), pkg("run_batch")
    T = 0.5
    base = ["--pairs", "1", "--size", "45x70", "--bcd-times", "2", "--thresh", "2", "--eval"]
    names = record_calls(monkeypatch)
    rb.main(base + ["--out", str(tmp_path / "a")])
    assert names == BATCH_FLOWS + ["dflow_fb_consistency"] + 4 * ["dflow_flow_eval"], "without the option: the calls it always issued"
    assert not (tmp_path / "a" / "margin_00.npy").exists()
    ja = json.load(open(tmp_path / "a" / "eval.json"))
    assert "confidence" not in ja and set(ja["pairs"][0]) == {"pair", "fwd", "sparse"}
    del names[:]
    capsys.readouterr()
    rb.main(base + ["--out", str(tmp_path / "b"), "--confidence", str(T)])
    assert names == (BATCH_FLOWS[:-2] + 2 * ["dflow_labels_to_flow", "dflow_label_confidence"] + ["dflow_fb_consistency"] + 2 * ["dflow_flow_gate"]
                     + 6 * ["dflow_flow_eval"])
    out = capsys.readouterr().out
    # the flows are those of the run without the option, byte for byte
    for name in (flowio.flow_name(0, 0, 2), flowio.flow_name(0, 1, 2), flowio.flow_name(0, 0, 2)[:-4] + ".flo"):
        assert open(tmp_path / "a" / name, "rb").read() == open(tmp_path / "b" / name, "rb").read(), name
    margin = np.load(tmp_path / "b" / "margin_00.npy")
    assert margin.dtype == np.float32 and margin.shape == (45, 70) and not np.isnan(margin).any()
    # the sparse field is the checked field of the other run, gated
    sparse_a, sparse_b = np.load(tmp_path / "a" / "sparse_field_00.npy"), np.load(tmp_path / "b" / "sparse_field_00.npy")
    want, (good, kept) = flow_gate_ref(sparse_a, margin, lo=T)
    assert np.array_equal(sparse_b.view(np.uint32), want.view(np.uint32)) and 0 < kept < good
    assert "pair 0: confidence gate at margin >= 0.5: %d of %d checked vectors stay" % (kept, good) in out
    jb = json.load(open(tmp_path / "b" / "eval.json"))
    assert jb["confidence"] == [T, "local", 1] and set(jb["pairs"][0]) == {"pair", "fwd", "sparse", "confident"}
    row = jb["pairs"][0]
    n_kept = int((margin >= np.float32(T)).sum())
    assert row["confident"]["n_test_valid"] == n_kept == jb["totals"]["confident"]["n_test_valid"] and 0 < n_kept < 45 * 70
    assert row["fwd"] == ja["pairs"][0]["fwd"] and row["sparse"]["n_test_valid"] == kept
