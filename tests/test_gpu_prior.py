"""dflow_prior_proposals and dflow_flow_advance on the device against their numpy definitions (tests/prior_ref.py), bit for
bit, and the layers above them.  The state comes from the package's own front end (load_pair, generisi, nasumicni) on
synth.make_pair; the expectation is prior_ref applied to what the device held before the step.
Everything here needs a real MI355X: run with `pytest -m gpu`."""
import numpy as np
import pytest

import prior_ref as R
from call_log import BACK, FRONT, record_calls
from conftest import pkg

pytestmark = pytest.mark.gpu

# (H, W, cellh, cellw, amp_x, amp_y): 45x35 has 1575 pixels, a multiple of neither 4 (pixels per wave) nor 16 (per block)
GEOMS = {"40x48": (40, 48, 5, 6, 4.0, 2.0), "45x35": (45, 35, 9, 7, 6.0, 3.0)}
SEED = 7


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


class Pass:
    """One front-end run, kept: the pass, clones of its four state tensors to start every case from, and the host copies the
    reference works on (full label pitch, fills included)."""

    def __init__(self, synth, geom, f16=False, seed=SEED, swap=False, **over):
        H, W, ch, cw, ax, ay = GEOMS[geom]
        L = pkg("_lib")
        if f16:
            over["flags"] = L.FLAG_DESCR_F16
        self.img1, self.img2, gt = synth.make_pair(H, W, seed=seed, amp_x=ax, amp_y=ay)
        if swap:
            self.img1, self.img2 = self.img2, self.img1
        self.gt = np.ascontiguousarray(gt, dtype=np.float32)                   # (H,W,2) [dy,dx]: the pair's true flow
        self.df = df = pkg("pipeline").DiscreteFlow(H, W, ch, cw, seed=seed, **over)
        df.load_pair(self.img1, self.img2)
        df.generisi()
        df.nasumicni()
        self.saved = [t.clone() for t in (df.proposals, df.lcosts, df.nprop, df.bestlabels)]
        self.d1, self.d2 = df.descriptors_f32(0).cpu().numpy(), df.descriptors_f32(1).cpu().numpy()
        self.H, self.W = H, W

    def restore(self):
        df = self.df
        for dst, src in zip((df.proposals, df.lcosts, df.nprop, df.bestlabels), self.saved):
            dst.copy_(src)
        df._bcd_ready = False

    def host(self):
        """The saved state as the reference takes it: uint32 / float32 (H,W,LP) and int64 (H,W) copies."""
        pr, lc, npr, bl = (t.cpu().numpy() for t in self.saved)
        return pr.view(np.uint32).copy(), lc.copy(), npr.astype(np.int64), bl.astype(np.int64)

    def device(self):
        df = self.df
        return (df.proposals.cpu().numpy().view(np.uint32), df.lcosts.cpu().numpy(), df.nprop.cpu().numpy().astype(np.int64),
                df.bestlabels.cpu().numpy().astype(np.int64))

    def uvv(self, dydx, holes=True):
        """[dy,dx] -> [U,V,valid], with a block of invalid pixels."""
        out = np.concatenate([dydx[..., ::-1], np.ones(dydx.shape[:2] + (1,), np.float32)], axis=-1).astype(np.float32)
        if holes:
            out[3:9, 5:11, 2] = 0.0
        return np.ascontiguousarray(out)

    def check(self, prior, stride, seed_labels=True, restore=True):
        """Runs the step on the device and the reference on the saved state; compares everything bit for bit.  Returns the
        reference's counts and state."""
        df = self.df
        if restore:
            self.restore()
        ref = self.host()
        want = R.prior_proposals(*ref, self.d1, self.d2, prior, stride, R.SEED_LABELS if seed_labels else 0, df.p.maxnprop, df.p.tphi)
        got = df.prior_proposals(prior, stride=stride, seed_labels=seed_labels, counts=True).cpu().tolist()
        dev = self.device()
        assert sum(want) == self.H * self.W * (5 if stride else 1)
        assert got == want, "counts"
        for name, a, b in zip(("proposals", "lcosts", "nprop", "bestlabels"), dev, ref):
            a32, b32 = (a.view(np.uint32), b.view(np.uint32)) if a.dtype == np.float32 else (a, b)
            assert a32.shape == b32.shape and np.array_equal(a32, b32), name
        assert not df._bcd_ready, "the compat lists must be rebuilt after the step"
        return want, ref


_passes = {}


@pytest.fixture
def get_pass(torch_, synth):
    def get(geom, f16=False, **over):
        key = (geom, f16, tuple(sorted(over.items())))
        if key not in _passes:
            _passes[key] = Pass(synth, geom, f16, **over)
        return _passes[key]
    return get


@pytest.mark.parametrize("layout", ["dydx", "uvv"])
@pytest.mark.parametrize("stride", [0, 2, 7])
@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("geom", list(GEOMS))
def test_prior_step_matches_the_reference(get_pass, geom, f16, stride, layout):
    ps = get_pass(geom, f16)
    prior = ps.gt if layout == "dydx" else ps.uvv(ps.gt)
    counts, _ = ps.check(prior, stride)
    assert counts[0] > 0 and counts[1] > 0, counts


@pytest.mark.parametrize("stride", [0, 2])
def test_small_label_budget_takes_every_branch(get_pass, stride):
    """window 0, ngauss 2, maxnprop 7, label_pitch 16: rows fill up, so appended, found, full and skipped all occur.
    Measured on this pass's state (the package's front end, sampler seed 7): stride 0: 825 / 895 / 132 / 68, stride 2:
    1501 / 5516 / 1962 / 621."""
    ps = get_pass("40x48", window=0, ngauss=2, maxnprop=7, label_pitch=16)
    counts, (_, _, npr, _) = ps.check(ps.gt, stride)
    print("small budget, stride %d: appended %d, found %d, full %d, skipped %d" % ((stride,) + tuple(counts)))
    assert all(c > 0 for c in counts), counts
    assert npr.max() == 7


def crafted_prior(H, W):
    """(H,W,3) [U,V,valid]: zero and valid, with one special vector per pixel along a few rows."""
    f = np.zeros((H, W, 3), np.float32)
    f[..., 2] = 1.0
    special = [np.nan, np.inf, -np.inf, 1e9, 32768.0, -32768.0, 0.5, -0.5, 1.5, 2.5, -2.5, 32767.4, 32767.6, 3.5, -1.5, 0.49999997]
    for i, v in enumerate(special):
        f[10, 4 + 2 * i, 0] = v                            # as U
        f[12, 4 + 2 * i, 1] = v                            # as V
    for i, x in enumerate((3, 20, 44)):                    # targets one pixel inside and one outside every border
        y = 20 + 2 * i
        f[y, x, :2] = (-x, 0);             f[y + 1, x, :2] = (-x - 1, 0)
        f[y, x + 1, :2] = (W - 2 - x, 0);  f[y + 1, x + 1, :2] = (W - 1 - x, 0)
        f[y, x + 2, :2] = (0, -y);         f[y + 1, x + 2, :2] = (0, -y - 2)
        f[y, x + 3, :2] = (0, H - 1 - y);  f[y + 1, x + 3, :2] = (0, H - 1 - y)
    for i, valid in enumerate((0.0, 0.5, 0.50001, np.nan, -1.0, 1.0)):
        f[30, 5 + 3 * i] = (2.0, 1.0, valid)
    return f


@pytest.mark.parametrize("stride", [0, 2])
def test_crafted_prior(get_pass, stride):
    ps = get_pass("40x48")
    f = crafted_prior(ps.H, ps.W)
    # the crafted vectors do what they were made for
    assert R.usable_vector(f, R.UVV, 10, 4 + 2 * 12) is None and R.usable_vector(f, R.UVV, 10, 4 + 2 * 11) == (0, 32767)
    assert R.usable_vector(f, R.UVV, 30, 8) is None and R.usable_vector(f, R.UVV, 30, 11) == (1, 2)
    counts, _ = ps.check(f, stride)
    assert counts[3] > 0, counts
    counts, _ = ps.check(np.ascontiguousarray(f[..., 1::-1]), stride)        # the same vectors as [dy,dx], every pixel valid
    assert counts[3] > 0, counts


def test_constant_field_appends_one_label(get_pass):
    ps = get_pass("40x48")
    prior = np.zeros((ps.H, ps.W, 2), np.float32)
    prior[..., 0], prior[..., 1] = -9.0, 11.0
    before = ps.host()[2]
    counts, (_, _, npr, _) = ps.check(prior, 2)
    assert (npr - before).max() == 1 and counts[0] == (npr - before).sum() > 0 and counts[1] > 0 and counts[3] > 0


def test_seed_flag_and_repeat(get_pass):
    ps = get_pass("45x35")
    before = ps.host()
    counts, ref = ps.check(ps.gt, 2, seed_labels=False)
    assert np.array_equal(ref[3], before[3]) and counts[0] > 0, "without the flag bestlabels is untouched"
    assert np.array_equal(ps.device()[3], before[3])
    ps.check(ps.gt, 2)
    state = [a.copy() for a in ps.device()]
    again = ps.df.prior_proposals(ps.gt, stride=2, counts=True).cpu().tolist()
    assert again[0] == 0 and again[2:] == [c for c in counts[2:]] and again[1] == counts[0] + counts[1]
    for a, b in zip(state, ps.device()):
        assert a.tobytes() == b.tobytes(), "a second identical call changes nothing"


def test_reach_beyond_the_search_window(get_pass):
    ps = get_pass("40x48")
    pr, _, npr, _ = ps.host()
    used = np.arange(pr.shape[2])[None, None, :] < npr[..., None]
    dx = (pr >> 16).astype(np.uint16).view(np.int16)
    assert np.abs(dx[used]).max() <= 17, "the kNN window ends at 17 px on this geometry"
    prior = np.zeros((ps.H, ps.W, 2), np.float32)
    prior[..., 1] = 20.0
    ps.check(prior, 0)
    flow = ps.df.vratiKonacniFlow().cpu().numpy()
    assert (flow[:, :28, 1] == 20).all() and (flow[:, :28, 0] == 0).all()
    assert (np.abs(flow[:, 28:, 1]) <= 17).all(), "x + 20 leaves the frame there: skipped"


@pytest.mark.parametrize("maxnprop", [150, 160])
def test_bcd_sweeps_after_the_prior_step_match_the_oracle(get_pass, oracle, maxnprop):
    """The lists and chain kernels take the longer rows."""
    O = oracle
    ps = get_pass("40x48", maxnprop=maxnprop)
    df = ps.df
    ps.check(ps.gt, 2)
    st = df.host_state()
    assert st["nprop"].max() > ps.host()[2].max()
    H, W, ch, cw = GEOMS["40x48"][:4]
    p = O.make_params(H, W, ch, cw, seed=SEED, maxnprop=maxnprop)
    bl = st["bestlabels"].copy()
    for sweep in range(2):
        df.ceoBCD(1)
        O.bcd_sweep(p, st["proposals"], st["lcosts"], st["nprop"], bl)
        assert np.array_equal(df.bestlabels.cpu().numpy(), bl), sweep


def test_batched_sweeps_of_two_seeded_passes_equal_separate_runs(torch_, synth, get_pass):
    a = get_pass("40x48")
    b = Pass(synth, "40x48", swap=True)                    # the backward pass of the same pair
    prior_b = pkg("pipeline").flow_advance(a.gt, negate=True)
    separate = []
    for ps, prior in ((a, a.gt), (b, prior_b)):
        ps.restore()
        ps.df.prior_proposals(prior, stride=2)
        ps.df.ceoBCD(2)
        separate.append(ps.df.bestlabels.cpu().numpy().copy())
    for ps, prior in ((a, a.gt), (b, prior_b)):
        ps.restore()
        ps.df.prior_proposals(prior, stride=2)
    pkg("pipeline").ceoBCD_batch([a.df, b.df], 2)
    for ps, want in zip((a, b), separate):
        assert np.array_equal(ps.df.bestlabels.cpu().numpy(), want)


def test_run_without_a_prior_issues_the_calls_it_always_did(get_pass, monkeypatch):
    ps = get_pass("40x48")
    names = record_calls(monkeypatch)
    flow0 = ps.df.run(ps.img1, ps.img2, 2).cpu().numpy().copy()
    assert names == FRONT + BACK
    del names[:]
    flow1 = ps.df.run(ps.img1, ps.img2, 2, prior=None, prior_stride=5).cpu().numpy().copy()
    assert names == FRONT + BACK and np.array_equal(flow0, flow1)
    del names[:]
    ps.df.run(ps.img1, ps.img2, 2, prior=ps.gt)
    assert names == FRONT + ["dflow_prior_proposals"] + BACK


def same_state(a, b):
    sa, sb = a.host_state(), b.host_state()
    return all(np.array_equal(sa[k], sb[k]) for k in ("proposals", "lcosts", "nprop", "bestlabels"))


def test_front_end_is_its_stages_called_by_hand(torch_, synth, monkeypatch):
    """DiscreteFlow.front_end on one object against load_pair, generisi, nasumicni[, prior_proposals] on another: the calls
    and the state, without a prior, with one, and with pack=True, after which ceoBCD does not build the matrices again."""
    H, W, ch, cw, ax, ay = GEOMS["40x48"]
    P = pkg("pipeline")
    img1, img2, gt = synth.make_pair(H, W, seed=SEED, amp_x=ax, amp_y=ay)
    prior = np.ascontiguousarray(gt, dtype=np.float32)
    df, hand = (P.DiscreteFlow(H, W, ch, cw, seed=SEED) for _ in range(2))

    def by_hand(**prior_args):
        hand.load_pair(img1, img2)
        hand.generisi()
        hand.nasumicni()
        return hand.prior_proposals(prior, **prior_args) if prior_args else None

    names = record_calls(monkeypatch)
    assert df.front_end(img1, img2) is None
    assert names == FRONT
    by_hand()
    assert same_state(df, hand)
    del names[:]
    cnt = df.front_end(img1, img2, prior=prior, prior_stride=3, seed_labels=False, counts=True)
    assert names == FRONT + ["dflow_prior_proposals"]
    want = by_hand(stride=3, seed_labels=False, counts=True)
    assert cnt.cpu().tolist() == want.cpu().tolist() and cnt.cpu().tolist()[0] > 0, "the prior appended labels"
    assert same_state(df, hand)
    del names[:]
    assert df.front_end(img1, img2, pack=True) is None
    assert names == FRONT + ["dflow_bcd_prepare"]
    del names[:]
    assert df.front_end(img1, img2, prior=prior, pack=True) is None, "no counts asked for"
    assert names == FRONT + ["dflow_prior_proposals", "dflow_bcd_prepare"]
    by_hand(stride=2)
    assert same_state(df, hand), "the defaults are prior_proposals' own: stride 2, seeded labels"
    del names[:]
    df.ceoBCD(2)
    assert names == 2 * ["dflow_bcd_sweep"], "packed by the front end: no second dflow_bcd_prepare"
    hand.ceoBCD(2)
    assert same_state(df, hand)


@pytest.mark.parametrize("negate", [False, True])
@pytest.mark.parametrize("layout", ["dydx", "uvv"])
@pytest.mark.parametrize("size", [(1, 1), (7, 9), (45, 35), (64, 257)])
def test_flow_advance_matches_the_reference(torch_, size, layout, negate):
    H, W = size
    rng = np.random.default_rng(H * 1000 + W)
    amp = max(1, min(H, W) // 3)
    flow = (rng.integers(-amp, amp + 1, (H, W, 2)) + rng.choice([0.0, 0.5], (H, W, 2), p=[0.7, 0.3])).astype(np.float32)
    if H * W > 1:
        flow[0, 0] = (0.0, -0.0)
        flow[H - 1, W - 1] = (np.nan, 1.0)
    if layout == "uvv":
        flow = np.concatenate([flow[..., ::-1], (rng.random((H, W, 1)) > 0.2).astype(np.float32)], axis=-1)
    flow = np.ascontiguousarray(flow)
    want, counts = R.flow_advance(flow, R.NEGATE if negate else 0)
    assert sum(counts) == H * W
    if H * W > 1:                                          # one pixel can neither lose a collision nor stay unclaimed beside a claimed one
        assert counts[1] > 0 and H * W - counts[0] > 0, counts
    got, cnt = pkg("pipeline").flow_advance(flow, negate=negate, counts=True)
    assert cnt.cpu().tolist() == counts
    got = got.cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    again = pkg("pipeline").flow_advance(torch_.from_numpy(flow).cuda(), negate=negate).cpu().numpy()
    assert again.tobytes() == got.tobytes()


def test_cli_prior_and_labels_options(torch_, synth, tmp_path, monkeypatch):
    """`daisy i flann.py --prior` then `python bcd.py --labels`: the files equal the in-process result."""
    import os
    import runpy
    import sys
    from conftest import PKG, ROOT
    H, W, ch, cw = 40, 48, 5, 6
    img1, img2, gt = synth.make_pair(H, W, seed=synth.pair_seed(3, 0))
    prior = np.clip(gt, -12, 12).astype(np.float32)
    monkeypatch.chdir(tmp_path)
    np.save("P.npy", prior)
    monkeypatch.setattr(sys, "argv", ["daisy i flann.py", "3", "0", "1", "--synthetic", "%dx%d" % (H, W), "--cell", "%dx%d" % (ch, cw),
                                      "--prior", "P.npy"])
    runpy.run_path(os.path.join(ROOT, PKG, "daisy i flann.py"), run_name="__main__")
    labels_file = "Daisy output slike 103 backward=0 labels_prior.npy"
    monkeypatch.setattr(sys, "argv", ["python bcd.py", "3", "0", "2", "--cell", "%dx%d" % (ch, cw), "--labels", labels_file])
    runpy.run_path(os.path.join(ROOT, PKG, "python bcd.py"), run_name="__main__")
    df = pkg("pipeline").DiscreteFlow(H, W, ch, cw)
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
