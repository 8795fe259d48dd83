"""dflow_pyr_down and dflow_flow_upsample on the device against their numpy definitions (tests/pyramid_ref.py), bit for bit,
and the layers above them: PyramidFlow against the same run composed on the CPU (the oracle's stages, pyramid_ref, prior_ref),
run_batch.py --pyramid and the two CLIs.
Everything here needs a real MI355X: run with `pytest -m gpu`."""
import os
import runpy
import sys

import numpy as np
import pytest

import pyramid_ref as R
from call_log import BACK, BATCH_PASS, FRONT, record_calls
from conftest import PKG, ROOT, pkg

pytestmark = pytest.mark.gpu

# 64x257: the coarse level is 32x129, three tiles wide (a seam at 64 and at 128, the last tile one pixel wide) and two tall;
# 45x35 -> 23x18: partial in both directions, odd rows of 105 bytes (every byte shift of a row start occurs)
SIZES = [(1, 1), (2, 3), (7, 9), (45, 35), (64, 257)]
BIG = (436, 1024)


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def image(kind, h, w, seed=0):
    if kind == "random":
        return np.random.default_rng(1000 * h + w + seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "white":
        return np.full((h, w, 3), 255, np.uint8)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return np.ascontiguousarray(np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2))      # one-pixel checkerboard


# every small size with every kind of image; the large frame once
DOWN_CASES = [(s, k) for s in SIZES for k in ("random", "white", "checker")] + [(BIG, "random")]


@pytest.mark.parametrize("size,kind", DOWN_CASES, ids=["%dx%d-%s" % (s + (k,)) for s, k in DOWN_CASES])
def test_pyr_down_matches_the_reference(torch_, size, kind):
    h, w = size
    P = pkg("pipeline")
    a, b = image(kind, h, w), image("random", h, w, seed=1)
    want_a, want_b = R.pyr_down(a), R.pyr_down(b)
    one = P.pyr_down(a).cpu().numpy()
    assert one.shape == want_a.shape and one.dtype == np.uint8 and np.array_equal(one, want_a)
    if kind == "white":
        assert (one == 255).all()
    ga, gb = (t.cpu().numpy() for t in P.pyr_down(torch_.from_numpy(a).cuda(), torch_.from_numpy(b).cuda()))
    assert np.array_equal(ga, want_a) and np.array_equal(gb, want_b), "the pair"
    assert ga.tobytes() == one.tobytes() and gb.tobytes() == P.pyr_down(b).cpu().numpy().tobytes(), "the pair's planes equal two single calls"


def coarse_flow(h, w, layout):
    """A random coarse flow for fine size (h,w): under [U,V,valid] a random 30 % invalid, and in both layouts a few crafted
    components: NaN, +-inf, and values whose sum or double overflows."""
    hc, wc = R.coarse_size(h, w)
    rng = np.random.default_rng(7 * h + w)
    f = rng.normal(0, 6, (hc, wc, 3)).astype(np.float32)
    f[..., 2] = rng.random((hc, wc)) > 0.3
    special = [np.nan, np.inf, -np.inf, 3e38, -3e38, 1.5e38, 2e38, -2e38]
    n = hc * wc
    for i, v in enumerate(special):
        if n > 2 * len(special):
            f.reshape(-1, 3)[(i * 2654435761) % n, i % 2] = v
            f.reshape(-1, 3)[(i * 2654435761) % n, 2] = 1.0
    if n > 40:                                                          # two large neighbours in a row: a + b overflows, 2a may not
        f[hc // 2, wc // 2 - 1] = (1.5e38, -2e38, 1.0)
        f[hc // 2, wc // 2] = (3e38, -2e38, 1.0)
    if layout == "dydx":
        f = f[..., 1::-1]
    return np.ascontiguousarray(f)


@pytest.mark.parametrize("layout", ["uvv", "dydx"])
@pytest.mark.parametrize("size", SIZES + [BIG], ids=lambda s: "%dx%d" % s)
def test_flow_upsample_matches_the_reference(torch_, size, layout):
    h, w = size
    P = pkg("pipeline")
    f = coarse_flow(h, w, layout)
    want, counts = R.flow_upsample(f, (h, w))
    assert sum(counts) == h * w
    if h * w > 1000:
        assert all(c > 0 for c in counts), counts
    got, cnt = P.flow_upsample(f, (h, w), counts=True)
    assert cnt.cpu().tolist() == counts
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    again = P.flow_upsample(torch_.from_numpy(f).cuda(), (h, w)).cpu().numpy()
    assert again.tobytes() == got.tobytes()


# ---- PyramidFlow against the run composed on the CPU
COMPOSE = {"40x48": (40, 48, 5, 6, 4.0, 2.0, 2), "45x35": (45, 35, 9, 7, 6.0, 3.0, 2), "40x48x3": (40, 48, 5, 6, 4.0, 2.0, 3)}
SEED = 7


def check_against_cpu(O, synth, case, f16=False, **over):
    H, W, ch, cw, ax, ay, nlev = COMPOSE[case]
    P, L = pkg("pipeline"), pkg("_lib")
    img1, img2, _ = synth.make_pair(H, W, seed=SEED, amp_x=ax, amp_y=ay)
    if f16:
        over["flags"] = L.FLAG_DESCR_F16
    pf = P.PyramidFlow(H, W, nlev, ch, cw, seed=SEED, **over)
    assert [pf.size(k) for k in range(nlev)] == [(H, W), ((H + 1) // 2, (W + 1) // 2), ((H + 3) // 4, (W + 3) // 4)][:nlev]
    flow = pf.run(img1, img2, 2, counts=True)
    want = R.compose(O, P.pyramid_levels(H, W, nlev, ch, cw, **over), img1, img2, 2, seed=SEED, f16=f16)
    for level in range(nlev - 1, -1, -1):                               # the coarsest first: the first difference is the cause
        df = pf.levels[level]
        assert np.array_equal(df.bestlabels.cpu().numpy(), want[level]["bestlabels"]), "labels of level %d" % level
        assert np.array_equal(df.flow.cpu().numpy().astype(np.float64), want[level]["flow"]), "flow of level %d" % level
    assert flow is pf.levels[0].flow
    got_counts = {lv: (u.cpu().tolist(), p.cpu().tolist()) for lv, u, p in pf.counts}
    assert got_counts == {lv: (want[lv]["upsample_counts"], want[lv]["prior_counts"]) for lv in range(nlev - 1)}
    assert want[0]["prior_counts"][0] > 0, "the prior appended labels"
    return pf


@pytest.mark.parametrize("case", list(COMPOSE))
def test_pyramid_run_equals_the_cpu_composition(torch_, oracle, synth, case):
    check_against_cpu(oracle, synth, case)


def test_pyramid_run_with_binary16_descriptors(torch_, oracle, synth):
    check_against_cpu(oracle, synth, "40x48", f16=True)


def test_pyramid_run_with_a_narrow_fine_window(torch_, oracle, synth):
    pf = check_against_cpu(oracle, synth, "40x48", fine_window=1)
    assert pf.levels[0].p.window == 1 and pf.levels[1].p.window == 2


# ---- reach
REACH, REACH_PIXELS = R.REACH, R.REACH_PIXELS        # tests/test_pyramid_compose.py recomputes the number on the CPU


def test_reach_beyond_the_window_of_every_level(torch_, synth):
    H, W, c, shift = REACH["H"], REACH["W"], REACH["cell"], REACH["shift"]
    P = pkg("pipeline")
    img1, img2 = R.reach_pair(synth)                                    # shifted by (0,+24), the edge replicated
    one = P.PyramidFlow(H, W, 1, c, c, seed=REACH["seed"], window=1)
    one.run(img1, img2, REACH["sweeps"])
    st = one.levels[0].host_state()
    used = np.arange(st["proposals"].shape[2])[None, None, :] < st["nprop"][..., None]
    assert np.abs(st["proposals"][..., 1][used]).max() <= 2 * c - 1, "window 1 and 8 px cells reach 15 px"
    assert not ((st["proposals"][..., 0] == 0) & (st["proposals"][..., 1] == shift) & used).any()
    two = P.PyramidFlow(H, W, 2, c, c, seed=REACH["seed"], window=1)
    flow = two.run(img1, img2, REACH["sweeps"]).cpu().numpy()
    n = int(((flow[..., 0] == 0) & (flow[..., 1] == shift)).sum())
    print("pixels at (0,%d): %d of %d with the target inside" % (shift, n, H * (W - shift)))
    assert n == REACH_PIXELS
    assert REACH_PIXELS > H * (W - shift) // 2


# ---- the calls
def test_one_level_issues_the_calls_of_a_plain_run(torch_, synth, monkeypatch):
    P = pkg("pipeline")
    H, W, ch, cw = 40, 48, 5, 6
    img1, img2, _ = synth.make_pair(H, W, seed=SEED, amp_x=4.0, amp_y=2.0)
    df = P.DiscreteFlow(H, W, ch, cw, seed=SEED)
    pf = P.PyramidFlow(H, W, 1, ch, cw, seed=SEED)
    names = record_calls(monkeypatch)
    plain = df.run(img1, img2, 2).cpu().numpy().copy()
    assert names == FRONT + BACK
    del names[:]
    got = pf.run(img1, img2, 2, coarse_bcd_times=5, prior_stride=3).cpu().numpy()
    assert names == FRONT + BACK and np.array_equal(got, plain)
    del names[:]
    P.PyramidFlow(H, W, 2, ch, cw, seed=SEED).run(img1, img2, 2, coarse_bcd_times=1)
    assert names == (["dflow_pyr_down"] + FRONT + ["dflow_bcd_prepare", "dflow_bcd_sweep", "dflow_labels_to_flow", "dflow_flow_upsample"]
                     + FRONT + ["dflow_prior_proposals"] + BACK)


BATCH_PLAIN = 2 * BATCH_PASS + 2 * ["dflow_bcd_sweep_batch"] + 2 * ["dflow_labels_to_flow"] + ["dflow_fb_consistency"]


def run_batch(tmp_path, *extra):
    rb = pkg("run_batch")
    rb.main(["--pairs", "1", "--size", "40x48", "--cell", "5x6", "--bcd-times", "2", "--out", str(tmp_path)] + list(extra))


def test_run_batch_without_pyramid_issues_the_calls_it_always_did(torch_, tmp_path, monkeypatch):
    names = record_calls(monkeypatch)
    run_batch(tmp_path / "a")
    assert names == BATCH_PLAIN
    del names[:]
    run_batch(tmp_path / "b", "--pyramid", "1")
    assert names == BATCH_PLAIN
    flowio = pkg("flowio")
    for backward in (0, 1):
        name = flowio.flow_name(0, backward, 2)
        assert np.array_equal(np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name))


@pytest.mark.parametrize("pyramid", [(), ("--pyramid", "2", "--coarse-bcd-times", "3")], ids=["plain", "pyramid"])
def test_run_batch_in_ragged_groups_writes_the_files_of_one_group(torch_, tmp_path, monkeypatch, pyramid):
    """4 passes as groups of 3 and 1 against one group of 4: what lies between two groups (the start event after the previous
    group's read-out, the first len(part) objects of the last group) changes no byte of any file."""
    rb = pkg("run_batch")
    names = record_calls(monkeypatch)
    for group in ("3", "4"):
        rb.main(["--pairs", "2", "--size", "40x48", "--cell", "5x6", "--bcd-times", "2", "--group", group,
                 "--out", str(tmp_path / group)] + list(pyramid))
        if group == "3" and not pyramid:
            assert names == (3 * BATCH_PASS + 2 * ["dflow_bcd_sweep_batch"] + 3 * ["dflow_labels_to_flow"]
                             + BATCH_PASS + 2 * ["dflow_bcd_sweep_batch"] + ["dflow_labels_to_flow"] + 2 * ["dflow_fb_consistency"])
    files = sorted(os.listdir(tmp_path / "3"))
    assert files == sorted(os.listdir(tmp_path / "4"))
    flowio = pkg("flowio")
    for pair in (0, 1):
        assert {flowio.flow_name(pair, 0, 2), flowio.flow_name(pair, 1, 2), "sparse_field_%02d.npy" % pair, "parovi_%02d.txt" % pair} <= set(files)
    for name in files:
        assert open(tmp_path / "3" / name, "rb").read() == open(tmp_path / "4" / name, "rb").read(), name


def test_run_batch_pyramid_equals_pyramid_flow(torch_, synth, tmp_path, monkeypatch):
    import json
    P, flowio = pkg("pipeline"), pkg("flowio")
    names = record_calls(monkeypatch)
    run_batch(tmp_path, "--pyramid", "2", "--coarse-bcd-times", "3", "--fine-window", "1", "--eval", "--photo", "--bcd-stats")
    level = BATCH_PASS[:3]
    assert names[:2 * 5 + 3 + 2 + 2] == (2 * (["dflow_pyr_down"] + BATCH_PASS) + 3 * ["dflow_bcd_sweep_batch"]
                                       + 2 * ["dflow_labels_to_flow", "dflow_flow_upsample"]), "the coarse level of both passes, batched"
    assert names[17:27] == 2 * (level + ["dflow_prior_proposals", "dflow_bcd_prepare"])
    del names[:]
    img1, img2, _ = synth.make_pair(40, 48, seed=synth.pair_seed(0, 0))
    for backward, (a, b) in enumerate(((img1, img2), (img2, img1))):
        pf = P.PyramidFlow(40, 48, 2, 5, 6, seed=0, fine_window=1)
        want = pf.run(a, b, 2, coarse_bcd_times=3).cpu().numpy().astype(np.float64)
        assert np.array_equal(np.load(tmp_path / flowio.flow_name(0, backward, 2)), want), backward
    for name in ("eval.json", "photo.json", "bcd_stats.json"):
        assert json.load(open(tmp_path / name))["pyramid"] == 2, name
    assert os.path.exists(tmp_path / "sparse_field_00.npy") and os.path.exists(tmp_path / "parovi_00.txt")


def test_the_two_clis_with_pyramid(torch_, synth, tmp_path, monkeypatch):
    """`daisy i flann.py --pyramid 2` then `python bcd.py --labels`: the files of --prior, equal to the in-process result."""
    H, W, ch, cw = 40, 48, 5, 6
    P = pkg("pipeline")
    img1, img2, _ = synth.make_pair(H, W, seed=synth.pair_seed(3, 0))
    monkeypatch.chdir(tmp_path)
    cli = os.path.join(ROOT, PKG, "daisy i flann.py")
    base = ["daisy i flann.py", "3", "0", "1", "--synthetic", "%dx%d" % (H, W), "--cell", "%dx%d" % (ch, cw)]
    monkeypatch.setattr(sys, "argv", base + ["--pyramid", "2", "--prior", "P.npy"])
    with pytest.raises(SystemExit):
        runpy.run_path(cli, run_name="__main__")
    monkeypatch.setattr(sys, "argv", base + ["--pyramid", "2", "--coarse-bcd-times", "3", "--fine-window", "1"])
    runpy.run_path(cli, run_name="__main__")
    labels_file = "Daisy output slike 103 backward=0 labels_prior.npy"
    monkeypatch.setattr(sys, "argv", ["python bcd.py", "3", "0", "2", "--cell", "%dx%d" % (ch, cw), "--labels", labels_file])
    runpy.run_path(os.path.join(ROOT, PKG, "python bcd.py"), run_name="__main__")
    pf = P.PyramidFlow(H, W, 2, ch, cw, fine_window=1)
    prior = pf.coarse_prior(pf.image_pyramid(img1, img2), 3)
    df = pf.levels[0]
    df.load_pair(img1, img2)
    df.generisi()
    wta = df.host_state()["bestlabels"]
    df.nasumicni()
    df.prior_proposals(prior, stride=2)
    st = df.host_state()
    for what, key in (("proposals_nakon_gausa", "proposals"), ("lcosts_nakon_gausa", "lcosts"), ("nprop", "nprop")):
        got = np.load("Daisy output slike 103 backward=0 %s.npy" % what)
        assert got.dtype == st[key].dtype and np.array_equal(got, st[key]), what
    seeded = np.load(labels_file)
    assert seeded.dtype == np.int64 and np.array_equal(seeded, st["bestlabels"]) and not np.array_equal(seeded, wta)
    assert np.array_equal(np.load("Bestlabels fajl slike 103 backward=0 posle 00 BCD.npy"), wta), '"posle 00" stays the kNN winner'
    df.ceoBCD(2)
    assert np.array_equal(np.load("Bestlabels fajl slike 103 backward=0 posle 02 BCD.npy"), df.bestlabels.cpu().numpy())
    assert np.array_equal(np.load("Gotova flow slika 103 backward=0 posle 02 BCD.npy"), df.vratiKonacniFlow().cpu().numpy().astype(np.float64))
    whole = P.PyramidFlow(H, W, 2, ch, cw, fine_window=1).run(img1, img2, 2, coarse_bcd_times=3).cpu().numpy()
    assert np.array_equal(whole, df.flow.cpu().numpy()), "the two CLIs together are PyramidFlow.run"
