"""Host-side mirror of the reference's hot path on one MI355X.

`DiscreteFlow` keeps the state the reference keeps in module globals (daisy i flann.py:89-95) as device
tensors and exposes the reference's own function names; each method is one call through the C-ABI
(include/dflow.h) on torch's current HIP stream.  torch is used for device memory, streams and
torch.distributed only -- every computation happens in libdflow.so.  No CPU fallback exists.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from . import bcdstats
from . import flowio

DEFAULT_CELLS = {  # (pich, picw) -> (cellh, cellw)
    (375, 1241): (25, 73),    # daisy i flann.py:34-35,42-43 (KITTI, exact tiling)
    (375, 1242): (25, 54),    # discrete_flow.py:22-23,30-31
    (436, 1024): (27, 64),    # Sintel: 16x16 cells, last cell row absorbs 4 rows
}


def default_cells(pich, picw):
    if (pich, picw) in DEFAULT_CELLS:
        return DEFAULT_CELLS[(pich, picw)]
    return max(5, pich // 15), max(5, picw // 17)   # the reference's 17x15 grid (daisy i flann.py:85-86)


class DiscreteFlow:
    """One (pair, direction) pass: DAISY -> kNN proposals -> neighbour proposals -> BCD sweeps."""

    def __init__(self, pich, picw, cellh=None, cellw=None, device="cuda:0", seed=0, **overrides):
        if not torch.cuda.is_available():
            raise _lib.DflowError("no HIP device visible: the dflow hot path has no CPU fallback")
        if cellh is None or cellw is None:
            cellh, cellw = default_cells(pich, picw)
        self.p = _lib.default_params(pich, picw, cellh, cellw, seed=seed, **overrides)
        self.ws_bytes = int(_lib.lib().dflow_workspace_bytes(C.byref(self.p)))
        _lib.check(0 if self.ws_bytes else -1, "dflow_workspace_bytes")
        self.device = torch.device(device)
        self._descr_f16 = bool(self.p.flags & _lib.FLAG_DESCR_F16)     # storage mode of the descriptor planes: fixed here
        H, W, LP = pich, picw, self.p.label_pitch
        dev = self.device
        # float32 (H,W,68), or with DFLOW_FLAG_DESCR_F16 binary16 (H,W,72): 68 values + 4 zero pads per pixel (include/dflow.h)
        self.descrs1 = self._new_descr()                                             # daisy i flann.py:80
        self.descrs2 = self._new_descr()                                             # :81
        self.proposals = torch.empty((H, W, LP), dtype=torch.int32, device=dev)     # :89 (packed int16 pairs)
        self.lcosts = torch.empty((H, W, LP), dtype=torch.float32, device=dev)      # :90
        self.nprop = torch.empty((H, W), dtype=torch.int32, device=dev)             # :91
        self.bestlabels = torch.empty((H, W), dtype=torch.int32, device=dev)        # :95
        self.flow = torch.empty((H, W, 2), dtype=torch.float32, device=dev)
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)
        self._img = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)          # staging of host images
        self._img2 = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
        self._bcd_ready = False     # compat matrices in the workspace are valid for the current proposals
        self._stats_ws = None       # workspace of dflow_bcd_stats(_batch), made by _bcd_stats_ws when first asked for

    # ------------------------------------------------------------------ helpers
    @property
    def descr_f16(self):
        return self._descr_f16

    def _new_descr(self):
        H, W = self.p.pich, self.p.picw
        if self.descr_f16:
            return torch.zeros((H, W, _lib.DESC_PITCH_F16), dtype=torch.float16, device=self.device)
        return torch.empty((H, W, 68), dtype=torch.float32, device=self.device)

    def _stream(self):
        return _lib.stream(self.device)

    def _pp(self):
        # the planes were allocated for one storage mode; a flag flipped afterwards would make the kernels read or write
        # 272-byte rows in 144-byte rows (or the reverse)
        if bool(self.p.flags & _lib.FLAG_DESCR_F16) != self._descr_f16:
            raise _lib.DflowError("DFLOW_FLAG_DESCR_F16 changed after construction: the descriptor planes are %s"
                                  % ("binary16 (H,W,72)" if self._descr_f16 else "float32 (H,W,68)"))
        return C.byref(self.p)

    def _state_args(self):
        """The tail of the front-end calls: the six state pointers, then workspace, its size and the stream."""
        return (self.descrs1.data_ptr(), self.descrs2.data_ptr(), self.proposals.data_ptr(), self.lcosts.data_ptr(),
                self.nprop.data_ptr(), self.bestlabels.data_ptr(), self.ws.data_ptr(), self.ws_bytes, self._stream())

    def _bcd_stats_ws(self, npass):
        """The workspace of dflow_bcd_stats(_batch) for npass passes like this one: kept here, grown when a larger batch asks."""
        per_pass = int(_lib.lib().dflow_bcd_stats_workspace_bytes(C.byref(self.p)))
        _lib.check(0 if per_pass else -1, "dflow_bcd_stats_workspace_bytes")
        need = per_pass * npass
        if self._stats_ws is None or self._stats_ws.numel() < need:
            self._stats_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._stats_ws, need

    # ------------------------------------------------------------------ reference-named stages
    def _device_image(self, picture, staging):
        """picture: (H,W,3) uint8 BGR, numpy (copied into the device tensor `staging`) or a contiguous device tensor."""
        t = _check(picture, "DiscreteFlow", "picture", torch.uint8, (self.p.pich, self.p.picw, 3))
        if isinstance(picture, np.ndarray):
            staging.copy_(t)
            return staging
        if not t.is_contiguous():
            raise ValueError("DiscreteFlow: picture must be a contiguous tensor")
        return t

    def izracunajDaisy(self, picture, out=None):
        """daisy i flann.py:69-77.  picture: (H,W,3) uint8 BGR (numpy or device tensor) -> (H,W,68) f32 tensor (with
        DFLOW_FLAG_DESCR_F16: (H,W,72) binary16, see descriptors_f32)."""
        img = self._device_image(picture, self._img)
        if out is None:
            out = self._new_descr()
        self._bcd_ready = False
        _lib.call("dflow_daisy", self._pp(), img.data_ptr(), out.data_ptr(), self.ws.data_ptr(), self.ws_bytes, self._stream())
        return out

    def load_pair(self, pic3, pic4):
        """daisy i flann.py:406-407: the descriptors of both images, in one set of launches (dflow_daisy_pair; the planes
        are bit for bit those of two izracunajDaisy calls)."""
        img1, img2 = self._device_image(pic3, self._img), self._device_image(pic4, self._img2)
        self._bcd_ready = False
        _lib.call("dflow_daisy_pair", self._pp(), img1.data_ptr(), img2.data_ptr(), self.descrs1.data_ptr(), self.descrs2.data_ptr(),
                  self.ws.data_ptr(), self.ws_bytes, self._stream())

    def set_descriptors(self, descrs1, descrs2):
        """(H,W,68) arrays -> the descriptor planes (rounded to binary16 if the pass stores them that way)."""
        for dst, src in ((self.descrs1, descrs1), (self.descrs2, descrs2)):
            dst[..., :68].copy_(torch.as_tensor(src, dtype=torch.float32).to(dst.dtype))

    def descriptors_f32(self, which):
        """Descriptors of image `which` (0: first, 1: second) as an (H,W,68) float32 tensor, whatever the storage."""
        return (self.descrs1, self.descrs2)[which][..., :68].to(torch.float32)

    def generisi(self):
        """napraviCD2 + generisi, daisy i flann.py:144-189."""
        self._bcd_ready = False
        _lib.call("dflow_knn_proposals", self._pp(), *self._state_args())

    KNN_KERNELS = ("basis", "prep", "knn_screen_kernel", "knn_resolve_kernel", "knn_fix_kernel", "knn_finalize_kernel")

    def generisi_timed(self):
        """generisi with HIP events between its kernels (dflow_knn_proposals_timed): returns ({kernel: ms}, MFMAs issued)."""
        self._bcd_ready = False
        ms = (C.c_float * 6)()
        issued = C.c_double()
        _lib.call("dflow_knn_proposals_timed", self._pp(), *self._state_args(), ms, C.byref(issued))
        return dict(zip(self.KNN_KERNELS, (float(v) for v in ms))), float(issued.value)

    KNN_STATS = ("lists_exact", "flags", "lists", "entries", "events", "max_entries_per_lane", "zero_queries", "bad_queries",
                 "zero_candidates", "zero_candidates_removed", "query_cell_pairs", "list_capacity", "heavy_pairs")
    KNN_STATS_ALL = KNN_STATS + ("heavy_pairs_left",)      # dflow_knn_screen_stats_n: DFLOW_KNN_STATS_ALL_N values

    def knn_stats(self):
        """dflow_knn_screen_stats_n: what the MFMA screen of the last generisi() did (call before the next stage reuses the workspace)."""
        out = (C.c_int64 * len(self.KNN_STATS_ALL))()
        _lib.call("dflow_knn_screen_stats_n", self._pp(), self.ws.data_ptr(), self.ws_bytes, self._stream(), out, len(out))
        st = dict(zip(self.KNN_STATS_ALL, (int(v) for v in out)))
        st["events_per_query_cell"] = round(st["events"] / max(1, st["query_cell_pairs"]), 3)
        return st

    def nasumicni(self):
        """daisy i flann.py:205-233."""
        self._bcd_ready = False
        _lib.call("dflow_neighbour_proposals", self._pp(), *self._state_args())

    def pakovanje(self):
        """daisy i flann.py:256-309: compat bit matrices, built into the workspace for the chain kernel."""
        _lib.call("dflow_bcd_prepare", self._pp(), self.proposals.data_ptr(), self.lcosts.data_ptr(),
                  self.nprop.data_ptr(), self.ws.data_ptr(), self.ws_bytes, self._stream())
        self._bcd_ready = True

    def bcd_phase(self, phase):
        """One of the four chain loops of ceoBCD, python bcd.py:265-277."""
        if not self._bcd_ready:
            self.pakovanje()
        _lib.call("dflow_bcd_phase", self._pp(), self.proposals.data_ptr(), self.nprop.data_ptr(), self.bestlabels.data_ptr(), phase,
                  self.ws.data_ptr(), self.ws_bytes, self._stream())

    def bcd_stats(self, prev=None, prev_out=None):
        """dflow_bcd_stats of the current labelling (DESIGN.md "BCD statistics and the stop rule"): its data and smoothness
        sums, and with prev, an (H,W) int32 device tensor of earlier labels, the number of labels that differ from it.
        prev_out, an (H,W) int32 device tensor (it may be prev itself), receives a copy of the labels.  Returns struct
        dflow_bcd_stats as a device tensor of 6 int64 words (bcd_stats_dict reads it back).  Runs on torch's current stream
        and does not wait for it; its small workspace is its own, the BCD records in self.ws stay valid."""
        H, W = self.p.pich, self.p.picw
        for name, t in (("prev", prev), ("prev_out", prev_out)):
            if t is not None and not (isinstance(t, torch.Tensor) and t.dtype == torch.int32 and tuple(t.shape) == (H, W)
                                      and t.is_contiguous() and t.device == self.device):
                raise ValueError("bcd_stats: %s must be a contiguous int32 (%d,%d) tensor on %s" % (name, H, W, self.device))
        ws, ws_bytes = self._bcd_stats_ws(1)
        out = torch.empty(6, dtype=torch.int64, device=self.device)
        _lib.call("dflow_bcd_stats", self._pp(), self.proposals.data_ptr(), self.lcosts.data_ptr(), self.nprop.data_ptr(),
                  self.bestlabels.data_ptr(), _ptr(prev), _ptr(prev_out), out.data_ptr(), ws.data_ptr(), ws_bytes, self._stream())
        return out

    def ceoBCD(self, bcd_times, on_sweep=None, stop=None):
        """python bcd.py:261-284.  on_sweep(w) is called after sweep w (the reference saves .npy there).
        stop=None: bcd_times sweeps and nothing else, returns None.  stop a dict with "changed_frac" and / or "rel_energy"
        (bcdstats.check_stop; an empty dict: statistics only): dflow_bcd_stats runs before the first sweep and after every
        sweep, and after every sweep its 48 bytes are read back -- the ONE synchronisation per sweep that a stop rule costs.
        The pass ends after the sweep with n_changed / (H*W) <= changed_frac, or with (E_prev - E) / E_prev <= rel_energy (a
        rise of E included: the labels kept are those of the sweep just done, nothing is rolled back), or after bcd_times
        sweeps.  Returns the history, a list of dicts (bcd_stats_dict plus "sweep"): entry 0 is the labelling before the
        first sweep (n_changed 0), entry w the one after sweep w."""
        stop = bcdstats.check_stop(stop)
        if not self._bcd_ready:
            self.pakovanje()
        if stop is not None:
            return ceoBCD_batch([self], bcd_times, on_sweep=on_sweep, stop=stop)[0]
        for w in range(1, bcd_times + 1):
            _lib.call("dflow_bcd_sweep", self._pp(), self.proposals.data_ptr(), self.nprop.data_ptr(), self.bestlabels.data_ptr(),
                      self.ws.data_ptr(), self.ws_bytes, self._stream())
            if on_sweep is not None:
                on_sweep(w)

    def vratiKonacniFlow(self, out=None):
        """python bcd.py:90-95: (H,W,2) [dy,dx] (float32 device tensor; values are small integers)."""
        out = self.flow if out is None else out
        _lib.call("dflow_labels_to_flow", self._pp(), self.proposals.data_ptr(), self.bestlabels.data_ptr(),
                  out.data_ptr(), self._stream())
        return out

    def prior_proposals(self, prior, stride=2, seed_labels=True, counts=False):
        """dflow_prior_proposals (DESIGN.md "Prior proposals"): appends the vectors of a flow somebody already has to the
        pixels' label sets, the pixel's own and, with stride > 0, those of the four pixels stride away, and with seed_labels
        starts the labelling on the pixel's own.  prior: (H,W,2) float32 [dy,dx] or (H,W,3) float32 [U,V,valid]; the last
        dimension says which.  Device tensor or host array; host data is uploaded to the pass's device.  Call it after
        nasumicni() (or set_host_state) and before the sweeps.  A prior only fills slots that are free (maxnprop - nprop per
        pixel).  Seed only a prior you believe: started on a wrong but smooth flow the sweeps stay on it.
        With counts=True returns the int32[4] device tensor {appended, found, full, skipped}, else None.  Runs on
        torch's current stream and does not wait for it."""
        prior = _check(prior, "prior_proposals", "prior", torch.float32, (self.p.pich, self.p.picw, (2, 3)))
        stride = int(stride)
        if not 0 <= stride <= 8192:
            raise ValueError("prior_proposals: stride must be in [0, 8192], got %d" % stride)
        prior, = _on(self.device, prior)
        cnt = _out(counts, 4, torch.int32, self.device)
        self._bcd_ready = False
        _lib.call("dflow_prior_proposals", self._pp(), self.descrs1.data_ptr(), self.descrs2.data_ptr(), prior.data_ptr(),
                  _layout(prior), stride, _lib.PRIOR_SEED_LABELS if seed_labels else 0, self.proposals.data_ptr(),
                  self.lcosts.data_ptr(), self.nprop.data_ptr(), self.bestlabels.data_ptr(), _ptr(cnt), self._stream())
        return cnt

    def confidence(self, mode="local", min_sep=1, thresh=None, alt=False, sparse=False, counts=False):
        """dflow_label_confidence of the current state (DESIGN.md "Label confidence"): per pixel the margin by which the chosen
        label's energy lies below the best competing motion of its own label set, a label competing when its flow is more than
        min_sep (0..1024, |.|_1) away from the chosen one.  mode "local": e_k = lamda * cost_k + the truncated-L1 smoothness
        against the four neighbours' chosen flows; "data": the matching cost alone (meaningful before any sweep).  Returns the
        (H,W) float32 device tensor (+Inf: no competitor, -Inf: no label in range), or a tuple in the order (margin[, alt][,
        sparse][, counts]): alt=True adds the (H,W) int32 plane of the competitor's slot (-1: none), sparse=True the (H,W,3)
        float32 [U,V,valid] field of the labelled pixels with margin >= thresh, counts=True the int32[6] device tensor
        LABEL_CONF_COUNTS.  thresh=None counts `kept` against -Inf (every labelled pixel) and refuses sparse=True.  Runs on
        torch's current stream and does not wait for it; the BCD records in self.ws stay valid."""
        mode, min_sep, thresh = _confidence_gate("confidence", mode, min_sep, thresh, sparse)
        H, W = self.p.pich, self.p.picw
        margin = torch.empty((H, W), dtype=torch.float32, device=self.device)
        extra = [_out(alt, (H, W), torch.int32, self.device), _out(sparse, (H, W, 3), torch.float32, self.device),
                 _out(counts, _lib.CONF_COUNTS, torch.int32, self.device)]
        _lib.call("dflow_label_confidence", self._pp(), self.proposals.data_ptr(), self.lcosts.data_ptr(), self.nprop.data_ptr(),
                  self.bestlabels.data_ptr(), mode, min_sep, thresh, margin.data_ptr(), _ptr(extra[0]), _ptr(extra[1]), _ptr(extra[2]),
                  self._stream())
        ret = tuple(t for t in [margin] + extra if t is not None)
        return ret if len(ret) > 1 else margin

    def front_end(self, pic3, pic4, prior=None, prior_stride=2, seed_labels=True, counts=False, pack=False):
        """Everything of a pass before its sweeps, daisy i flann.py main (:406-422, without the file writes): load_pair, generisi,
        nasumicni, with a prior prior_proposals(prior, prior_stride, seed_labels, counts), with pack=True pakovanje (for passes
        whose sweeps are batched: the compat matrices are then built here, on the front end's stream).  Returns what
        prior_proposals returned, None without a prior."""
        self.load_pair(pic3, pic4)
        self.generisi()
        self.nasumicni()
        cnt = None if prior is None else self.prior_proposals(prior, stride=prior_stride, seed_labels=seed_labels, counts=counts)
        if pack:
            self.pakovanje()
        return cnt

    def run(self, pic3, pic4, bcd_times, prior=None, prior_stride=2):
        """front_end followed by ceoBCD; returns the flow tensor.  prior: a flow to start from (prior_proposals, with seeded
        labels); None: the reference's pass."""
        self.front_end(pic3, pic4, prior, prior_stride)
        self.ceoBCD(bcd_times)
        return self.vratiKonacniFlow()

    # ------------------------------------------------------------------ reference dtypes on the host
    def host_state(self):
        """proposals int64 (H,W,150,2) / lcosts float64 / nprop, bestlabels int64, as the reference saves them
        (daisy i flann.py:249-253)."""
        L = self.p.maxnprop
        packed = self.proposals[..., :L].cpu().numpy().view(np.uint32)
        dy = (packed & 0xFFFF).astype(np.uint16).view(np.int16).astype(np.int64)
        dx = (packed >> 16).astype(np.uint16).view(np.int16).astype(np.int64)
        return dict(proposals=np.stack([dy, dx], axis=-1),
                    lcosts=self.lcosts[..., :L].cpu().numpy().astype(np.float64),
                    nprop=self.nprop.cpu().numpy().astype(np.int64),
                    bestlabels=self.bestlabels.cpu().numpy().astype(np.int64))

    def set_host_state(self, proposals, lcosts, nprop, bestlabels):
        """Upload reference-dtype arrays (ucitajSvePodatkeDoBCD, python bcd.py:67-81)."""
        L, LP = self.p.maxnprop, self.p.label_pitch
        H, W = self.p.pich, self.p.picw
        packed = np.full((H, W, LP), 0xFFFFFFFF, np.uint32)
        packed[..., :L] = (proposals[..., 0].astype(np.int16).view(np.uint16).astype(np.uint32)
                           | (proposals[..., 1].astype(np.int16).view(np.uint16).astype(np.uint32) << 16))
        lc = np.full((H, W, LP), 1000.0, np.float32)
        lc[..., :L] = lcosts.astype(np.float32)
        # the device keeps the data costs as float32: exact for everything the reference writes (min(tphi, a float32 sum),
        # daisy i flann.py:179-180,228-229) -- anything else would silently change the DP, so it is refused
        if not np.array_equal(lc[..., :L].astype(np.float64), lcosts):
            raise ValueError("lcosts holds values that are not float32-exact (the reference's files are): refusing to round them")
        # the costs of used slots lie in [0, tphi] (min(tphi, a sum of absolute values)); the bound that keeps the DP below
        # the reference's 800000 sentinels assumes it (include/dflow.h, DFLOW_DP_SENTINEL)
        used = np.arange(L)[None, None, :] < np.asarray(nprop)[..., None]
        cu = lcosts[..., :L][used]
        if not (np.isfinite(cu).all() and (cu >= 0).all() and (cu <= self.p.tphi).all()):
            raise ValueError("lcosts of used slots must lie in [0, tphi=%g]" % self.p.tphi)
        if proposals.min() < -32768 or proposals.max() > 32767:
            raise ValueError("proposals outside the int16 range of the packed device layout")
        self.proposals.copy_(torch.from_numpy(packed.view(np.int32)))
        self.lcosts.copy_(torch.from_numpy(lc))
        self.nprop.copy_(torch.from_numpy(nprop.astype(np.int32)))
        self.bestlabels.copy_(torch.from_numpy(bestlabels.astype(np.int32)))
        self._bcd_ready = False


def bcd_stats_dict(t, lamda, npix):
    """The one read-back of DiscreteFlow.bcd_stats: its statistics tensor -> a dict of struct dflow_bcd_stats's fields plus
    energy = lamda * data_sum + smooth_sum, formed here in double, and changed_frac = n_changed / npix, npix the pixel count
    H*W of the pass (the 48 bytes do not carry it)."""
    return bcdstats.stats_dict(t.cpu().numpy().tobytes(), lamda, int(npix))


def ceoBCD_batch(passes, bcd_times, on_sweep=None, stop=None):
    """ceoBCD (python bcd.py:261-284) for several independent passes at once (forward and backward runs of a pair, several
    pairs: README.md:40 of the reference): the chains of all passes share the four launches of a sweep.  `passes` are
    DiscreteFlow objects of identical geometry and constants on one device; results equal separate ceoBCD calls.
    stop as for DiscreteFlow.ceoBCD: None runs bcd_times sweeps with no other launch and returns None.  With a dict, one
    dflow_bcd_stats_batch follows every sweep (and one precedes the first), the 48 bytes per pass are read back together --
    one synchronisation per sweep -- and a pass whose rule fires leaves the later launches; on_sweep(w) is called while any
    pass still runs.  Returns one history per pass (see ceoBCD)."""
    passes = list(passes)
    stop = bcdstats.check_stop(stop)
    if not passes:
        return None if stop is None else []
    first = passes[0]

    def constants(p):
        return (p.pich, p.picw, p.cellh, p.cellw, p.tpsi, p.lamda, p.label_pitch, p.maxnprop)
    for df in passes:
        if constants(df.p) != constants(first.p):
            raise ValueError("batched passes must share geometry and constants")
        if df.device != first.device:
            raise ValueError("batched passes must live on one device")
        if not df._bcd_ready:
            df.pakovanje()

    def ptrs(active, get):
        return (C.c_void_p * len(active))(*[get(passes[i]).data_ptr() for i in active])

    def sweep_args(active):
        return len(active), ptrs(active, lambda d: d.nprop), ptrs(active, lambda d: d.bestlabels), ptrs(active, lambda d: d.ws)

    def stats(active, w):
        """dflow_bcd_stats_batch of the passes `active` (indices) against prevs, which then hold their labels; one read-back.
        Appends entry w to their histories and returns the indices of those that sweep w does not stop."""
        sws, sws_bytes = first._bcd_stats_ws(len(active))
        out = torch.empty((len(active), 6), dtype=torch.int64, device=first.device)
        _lib.call("dflow_bcd_stats_batch", first._pp(), len(active), ptrs(active, lambda d: d.proposals), ptrs(active, lambda d: d.lcosts),
                  ptrs(active, lambda d: d.nprop), ptrs(active, lambda d: d.bestlabels),
                  (C.c_void_p * len(active))(*[prevs[i].data_ptr() for i in active]), out.data_ptr(), sws.data_ptr(), sws_bytes,
                  first._stream())
        raw = out.cpu().numpy().tobytes()               # the synchronisation
        still = []
        for i, d in zip(active, bcdstats.stats_dicts(raw, first.p.lamda, first.p.pich * first.p.picw)):
            d["sweep"] = w
            if w == 0 or not bcdstats.should_stop(stop, d, histories[i][-1]["energy"]):
                still.append(i)
            histories[i].append(d)
        return still

    active = list(range(len(passes)))
    if stop is not None:
        if any(df.p.tphi != first.p.tphi for df in passes):
            raise ValueError("batched passes must share geometry and constants")
        histories = [[] for _ in passes]
        # entry 0, the labelling the sweeps start from: compared with itself (n_changed 0); its energy is the E_prev of sweep 1
        prevs = [df.bestlabels.clone() for df in passes]
        stats(active, 0)
    args = sweep_args(active)
    for w in range(1, bcd_times + 1):
        if not active:
            break
        _lib.call("dflow_bcd_sweep_batch", first._pp(), *args, first.ws_bytes, first._stream())
        if stop is not None:
            still = stats(active, w)
            if len(still) != len(active):
                active, args = still, sweep_args(still)
        if on_sweep is not None:
            on_sweep(w)
    return None if stop is None else histories


CONF_MODES = {"local": _lib.CONF_LOCAL, "data": _lib.CONF_DATA}
LABEL_CONF_COUNTS = ("labelled", "not_labelled", "no_alternative", "negative", "zero", "kept")


def _confidence_gate(fn, mode, min_sep, thresh, sparse=False):
    """The arguments of DiscreteFlow.confidence as the library takes them, (mode, min_sep, thresh), before any device is touched."""
    if mode not in CONF_MODES:
        raise ValueError("%s: mode must be 'local' or 'data', got %r" % (fn, mode))
    if not (isinstance(min_sep, (int, np.integer)) and 0 <= min_sep <= 1024):
        raise ValueError("%s: min_sep must be an int in [0, 1024], got %r" % (fn, min_sep))
    if thresh is None:
        if sparse:
            raise ValueError("%s: sparse=True needs a thresh" % fn)
        thresh = float("-inf")
    if not isinstance(thresh, (int, float, np.integer, np.floating)) or np.isnan(np.float32(thresh)):
        raise ValueError("%s: thresh must be a number, not NaN, got %r" % (fn, thresh))
    return CONF_MODES[mode], int(min_sep), float(np.float32(thresh))


def fb_consistency(fwd, bwd, tresh, p=None):
    """postProcessing (postprocessing.py:123-135) on two (H,W,2) [dy,dx] float32 device tensors ->
    (H,W,3) float32 [U,V,valid] device tensor."""
    H, W, _ = fwd.shape
    if p is None:
        ch, cw = default_cells(H, W)
        p = _lib.default_params(H, W, ch, cw)
    out = torch.empty((H, W, 3), dtype=torch.float32, device=fwd.device)
    _lib.call("dflow_fb_consistency", C.byref(p), fwd.contiguous().data_ptr(), bwd.contiguous().data_ptr(),
              float(tresh), out.data_ptr(), _lib.stream(fwd.device))
    return out


# ---------------------------------------------------------------------- image-plane stages: what every wrapper below shares
def _check(a, fn, name, dtype, shape):
    """The input gate: an array or tensor -> the tensor, as it is (no copy of a tensor, no device touched), if it has `dtype`
    and fits `shape`: one entry per dimension, None for any size, a tuple for a choice of sizes.  ValueError otherwise."""
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    if t.dtype != dtype or t.dim() != len(shape) or any(
            want is not None and got not in (want if isinstance(want, tuple) else (want,)) for got, want in zip(t.shape, shape)):
        text = ",".join("HWC"[i] if want is None else "|".join(map(str, want)) if isinstance(want, tuple) else str(want)
                        for i, want in enumerate(shape))
        raise ValueError("%s: %s must be %s (%s), got %s %s" % (fn, name, str(dtype)[6:], text, tuple(t.shape), t.dtype))
    return t


def _device_of(*tensors):
    """The device of the first CUDA tensor among the arguments, else the current CUDA device."""
    for t in tensors:
        if t.is_cuda:
            return t.device
    return torch.device("cuda", torch.cuda.current_device())


def _on(dev, *tensors):
    """The tensors on `dev`, contiguous, each starting on a 16-byte boundary, the most include/dflow.h asks of a data plane.  A
    caller's device tensor that already is all that stays as it is; a contiguous view that starts lower (flows[1] of a stack of
    (H,W,3) fields whose H*W*12 is no multiple of 16) is cloned: an allocation starts on 256 bytes."""
    out = [t.to(dev).contiguous() for t in tensors]
    return [t.clone() if t.data_ptr() % 16 else t for t in out]


def _out(cond, shape, dtype, dev):
    return torch.empty(shape, dtype=dtype, device=dev) if cond else None


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _layout(flow):
    return _lib.EVAL_UVV if flow.shape[2] == 3 else _lib.EVAL_DYDX


def _stats_arg(stats, nwords, dev, fn):
    """The stats= argument of flow_eval / warp_eval -> (tensor, accumulate): a new tensor to overwrite, or the caller's."""
    if stats is None:
        return torch.empty(nwords, dtype=torch.int64, device=dev), False
    if not (isinstance(stats, torch.Tensor) and stats.dtype == torch.int64 and stats.numel() == nwords and stats.is_contiguous()
            and stats.device == dev):
        raise ValueError("%s: stats must be the int64[%d] tensor of an earlier call on %s" % (fn, nwords, dev))
    return stats, True


def _struct_dict(cls, t):
    """The read-back of a statistics tensor: struct `cls` of _lib -> a dict of its fields, ints and floats, without `reserved`."""
    s = cls.from_buffer_copy(t.cpu().numpy().tobytes())
    return {name: getattr(s, name) for name, _ in cls._fields_ if name != "reserved"}


def _pct(x, n):
    return x * 100 / n if n else float("nan")


def canny_edges(bgr, low=100, high=200, ivice=True):
    """canny_ivice, edge.py:19-35 (cv2.cvtColor BGR2GRAY -> cv2.GaussianBlur((3,3), 0) -> cv2.Canny(low, high)) on a (H,W,3)
    uint8 BGR image (numpy array or tensor; a host image is uploaded to the current device) -> (edges, ivice): device
    tensors (H,W) uint8 0/255 and (H,W) float32 (255 - edges) / 255, or None with ivice=False.  Runs on torch's current
    stream and does not wait for it."""
    bgr = _check(bgr, "canny_edges", "bgr", torch.uint8, (None, None, 3))
    dev = _device_of(bgr)
    bgr, = _on(dev, bgr)
    H, W, _ = bgr.shape
    ws, ws_bytes = _lib.workspace("dflow_canny_workspace_bytes", H, W, dev)
    edges = torch.empty((H, W), dtype=torch.uint8, device=dev)
    iv = _out(ivice, (H, W), torch.float32, dev)
    _lib.call("dflow_canny_edges", H, W, bgr.data_ptr(), float(low), float(high), edges.data_ptr(), _ptr(iv), ws.data_ptr(), ws_bytes,
              _lib.stream(dev))
    return edges, iv


def pb_edges(bgr, radius=5, per_orientation=False):
    """Soft edge strength without a trained model (dflow_pb_edges, DESIGN.md "Pb edge strength"): a Pb-style oriented half-disc
    histogram gradient of a (H,W,3) uint8 BGR image (numpy array or tensor; a host image is uploaded to the current device)
    with disc radius 1..7 -> the (H,W) float32 device tensor e in [0,1], the edge strength dflow_epic_interpolate and
    dflow_epic_prefilter are defined on; with per_orientation=True (e, m): m the (H,W,8) float32 responses of the 8
    orientations, e their maximum.  Runs on torch's current stream and does not wait for it."""
    bgr = _check(bgr, "pb_edges", "bgr", torch.uint8, (None, None, 3))
    dev = _device_of(bgr)
    bgr, = _on(dev, bgr)
    H, W, _ = bgr.shape
    ws, ws_bytes = _lib.workspace("dflow_pb_workspace_bytes", H, W, dev)
    e = torch.empty((H, W), dtype=torch.float32, device=dev)
    m = _out(per_orientation, (H, W, 8), torch.float32, dev)
    _lib.call("dflow_pb_edges", H, W, bgr.data_ptr(), int(radius), e.data_ptr(), _ptr(m), ws.data_ptr(), ws_bytes, _lib.stream(dev))
    return (e, m) if per_orientation else e


EPIC_METHODS = {"LA": 0, "NW": 1}     # DFLOW_EPIC_LA, DFLOW_EPIC_NW


def epic_interpolate(sparse, edges, nn=100, k=0.8, method="LA", aux=False, lists=True):
    """EpicFlow's sparse-to-dense step (dflow_epic_interpolate): a (H,W,3) float32 [U,V,valid] sparse field and a (H,W)
    float32 edge map (device tensors or host arrays; host data is uploaded to the current device) -> (H,W,2) float32 [dy,dx]
    device tensor.  nn neighbours per seed, kernel coefficient k, method "LA" (locally-weighted affine) or "NW"
    (Nadaraya-Watson).  With aux=True returns (flow, S, D, lists, list_g): S (H,W) int32 seed ids (-1 without seeds),
    D (H,W) int32 geodesic distances (the uint32 bits; -1 without seeds), lists (H*W, nn) int32 and list_g (H*W, nn) int64
    (-1 pads; None with lists=False: they take H*W*nn*12 bytes).  Runs on torch's current stream; the call synchronises
    that stream (the Voronoi loop reads a counter back)."""
    if method not in EPIC_METHODS:
        raise ValueError("epic_interpolate: method must be 'LA' or 'NW', not %r" % (method,))
    sparse = _check(sparse, "epic_interpolate", "sparse", torch.float32, (None, None, 3))
    H, W, _ = sparse.shape
    edges = _check(edges, "epic_interpolate", "edges", torch.float32, (H, W))
    dev = _device_of(sparse)
    sparse, edges = _on(dev, sparse, edges)
    ws, ws_bytes = _lib.workspace("dflow_epic_workspace_bytes", H, W, dev)
    flow = torch.empty((H, W, 2), dtype=torch.float32, device=dev)
    S, D = _out(aux, (H, W), torch.int32, dev), _out(aux, (H, W), torch.int32, dev)
    lst = _out(aux and lists, (H * W, int(nn)), torch.int32, dev)
    list_g = _out(aux and lists, (H * W, int(nn)), torch.int64, dev)
    _lib.call("dflow_epic_interpolate", H, W, sparse.data_ptr(), edges.data_ptr(), int(nn), float(k), EPIC_METHODS[method],
              flow.data_ptr(), _ptr(S), _ptr(D), _ptr(lst), _ptr(list_g), ws.data_ptr(), ws_bytes, _lib.stream(dev))
    return (flow, S, D, lst, list_g) if aux else flow


# EpicFlow's pre-filter defaults; recalled, not checked against the binary.
PREFILTER_DEFAULTS = dict(saliency_th=0.045, pref_nn=25, pref_th=5.0)


def epic_prefilter(sparse, edges, img1=None, saliency_th=None, pref_nn=25, pref_th=5.0, k=0.8, aux=False):
    """EpicFlow's match pre-filter (dflow_epic_prefilter, DESIGN.md "Match pre-filter"): a (H,W,3) float32 [U,V,valid] sparse
    field, a (H,W) float32 edge map and optionally the first image, (H,W,3) uint8 BGR (device tensors or host arrays; host
    data is uploaded to the current device) -> the (H,W,3) float32 device tensor with every dropped seed set to [0,0,0].
    Stage A drops seeds whose image saliency is below saliency_th (None: 0.045 with img1, 0 without; it needs the image, so
    a non-zero saliency_th with img1=None is a ValueError), stage B those whose flow is further than pref_th px from the
    Nadaraya-Watson estimate of their pref_nn nearest seeds (kernel coefficient k); 0 skips a stage.  The defaults are
    EpicFlow's as recalled, not checked against the binary.  With aux=True returns (filtered, reason, saliency, estimate):
    (H,W) uint8 0 no seed / 1 kept / 2 saliency / 3 consistency, (H,W) float32, (H,W,2) float32 [u^,v^].  The input is not
    modified.  Runs on torch's current stream; the call synchronises that stream."""
    if saliency_th is None:
        saliency_th = PREFILTER_DEFAULTS["saliency_th"] if img1 is not None else 0.0
    if img1 is None and saliency_th != 0:
        raise ValueError("epic_prefilter: saliency_th=%g needs img1 (without an image only saliency_th = 0 runs)" % saliency_th)
    sparse = _check(sparse, "epic_prefilter", "sparse", torch.float32, (None, None, 3))
    H, W, _ = sparse.shape
    edges = _check(edges, "epic_prefilter", "edges", torch.float32, (H, W))
    if img1 is not None:
        img1 = _check(img1, "epic_prefilter", "img1", torch.uint8, (H, W, 3))
    dev = _device_of(sparse)
    sparse, edges = _on(dev, sparse, edges)
    if img1 is not None:
        img1, = _on(dev, img1)
    ws, ws_bytes = _lib.workspace("dflow_epic_prefilter_workspace_bytes", H, W, dev)
    out = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    reason, saliency, estimate = _out(aux, (H, W), torch.uint8, dev), _out(aux, (H, W), torch.float32, dev), _out(aux, (H, W, 2), torch.float32, dev)
    _lib.call("dflow_epic_prefilter", H, W, _ptr(img1), sparse.data_ptr(), edges.data_ptr(), float(saliency_th), int(pref_nn),
              float(pref_th), float(k), out.data_ptr(), _ptr(reason), _ptr(saliency), _ptr(estimate), ws.data_ptr(), ws_bytes,
              _lib.stream(dev))
    return (out, reason, saliency, estimate) if aux else out


def epic_prefilter_last_stats():
    """({"seeds", "dropped_saliency", "dropped_consistency"}, {stage: ms}) of the last epic_prefilter on this thread."""
    counts, ms = (C.c_int32 * 3)(), (C.c_float * 4)()
    _lib.call("dflow_epic_prefilter_last_stats", counts, ms)
    return (dict(zip(("seeds", "dropped_saliency", "dropped_consistency"), (int(v) for v in counts))),
            dict(zip(("saliency", "graph", "consistency", "compact"), (float(v) for v in ms))))


# The variational part of EpicFlow's presets, as its documentation gives them; recalled, not checked against the binary.
VAR_PRESETS = {
    "sintel": dict(niter_outer=5, alpha=1.0, gamma=0.72, delta=0.0, sigma=1.1),
    "kitti": dict(niter_outer=2, alpha=1.0, gamma=0.77, delta=0.0, sigma=1.7),
    "middlebury": dict(niter_outer=25, alpha=1.0, gamma=0.72, delta=0.0, sigma=1.1),
}
_VAR_FIELDS = tuple(name for name, _ in _lib.VarParams._fields_)


def var_params(preset=None, **params):
    """struct dflow_var_params: the library's defaults, then the preset ("sintel", "kitti", "middlebury" or None), then the
    keyword arguments (the struct's field names).  ValueError for an unknown preset or field."""
    p = _lib.VarParams()
    _lib.lib().dflow_var_default_params(C.byref(p))
    if preset is not None and preset not in VAR_PRESETS:
        raise ValueError("variational_refine: preset must be one of %s or None, not %r" % (sorted(VAR_PRESETS), preset))
    for k, v in list(VAR_PRESETS.get(preset, {}).items()) + list(params.items()):
        if k not in _VAR_FIELDS:
            raise ValueError("variational_refine: unknown parameter %r (known: %s)" % (k, ", ".join(_VAR_FIELDS)))
        setattr(p, k, v)
    return p


def variational_refine(img1, img2, flow, preset=None, **params):
    """Variational refinement of a dense flow (dflow_var_refine, DESIGN.md "Variational refinement"): two (H,W,3) uint8 BGR
    images and a (H,W,2) float32 [dy,dx] flow (device tensors or host arrays; host data is uploaded to the current device)
    -> the refined (H,W,2) float32 [dy,dx] device tensor.  preset and params as in var_params (alpha, gamma, delta, sigma,
    sor_omega, niter_outer, niter_inner, niter_solver, flags).  Runs on torch's current stream and does not wait for it."""
    p = var_params(preset, **params)
    flow = _check(flow, "variational_refine", "flow", torch.float32, (None, None, 2))
    H, W, _ = flow.shape
    img1 = _check(img1, "variational_refine", "img1", torch.uint8, (H, W, 3))
    img2 = _check(img2, "variational_refine", "img2", torch.uint8, (H, W, 3))
    dev = _device_of(flow)
    flow, img1, img2 = _on(dev, flow, img1, img2)
    ws, ws_bytes = _lib.workspace("dflow_var_workspace_bytes", H, W, dev)
    out = torch.empty((H, W, 2), dtype=torch.float32, device=dev)
    _lib.call("dflow_var_refine", H, W, img1.data_ptr(), img2.data_ptr(), flow.data_ptr(), C.byref(p), out.data_ptr(),
              ws.data_ptr(), ws_bytes, _lib.stream(dev))
    return out


def epic_last_stats():
    """(Voronoi rounds, {stage: ms}) of the last epic_interpolate on this thread, from HIP events (waits for them)."""
    rounds, ms = C.c_int32(0), (C.c_float * 4)()
    _lib.call("dflow_epic_last_stats", C.byref(rounds), ms)
    return rounds.value, dict(zip(("voronoi", "graph", "lists", "fill"), (float(v) for v in ms)))


def flow_eval(test, gt, abs_thresh=3.0, err=False, image=False, stats=None):
    """errorImage, visualization.py:128-156, on the GPU (dflow_flow_eval, DESIGN.md "Flow evaluation"): the end-point error
    of `test` against the ground truth `gt`, (H,W,3) float32 [U,V,valid].  test is (H,W,3) float32 [U,V,valid] (what
    fb_consistency and evaluate.ucitajFlow give) or (H,W,2) float32 [dy,dx] with every pixel valid (what the dense stages
    write); the last dimension says which.  Device tensors or host arrays; host data is uploaded to the current device.
    Returns the statistics as a device tensor (struct dflow_eval_stats as 8 int64 words; eval_stats reads it back), then, if
    asked for, err: (H,W) float32, the error at the compared pixels and -1 elsewhere, and image: (H,W,3) uint8, the reference's
    colour picture in BGR order.  stats: the tensor of an earlier call (or torch.zeros(8, int64)) to add this field's values
    to, so that a batch is totalled on the device.  Runs on torch's current stream and does not wait for it."""
    gt = _check(gt, "flow_eval", "gt", torch.float32, (None, None, 3))
    H, W, _ = gt.shape
    test = _check(test, "flow_eval", "test", torch.float32, (H, W, (2, 3)))
    dev = _device_of(test, gt)
    test, gt = _on(dev, test, gt)
    stats, accumulate = _stats_arg(stats, 8, dev, "flow_eval")
    ws, ws_bytes = _lib.workspace("dflow_eval_workspace_bytes", H, W, dev)
    e, img = _out(err, (H, W), torch.float32, dev), _out(image, (H, W, 3), torch.uint8, dev)
    _lib.call("dflow_flow_eval", H, W, test.data_ptr(), _layout(test), gt.data_ptr(), float(abs_thresh),
              _lib.EVAL_FLAG_ACCUMULATE if accumulate else 0, stats.data_ptr(), _ptr(e), _ptr(img), ws.data_ptr(), ws_bytes,
              _lib.stream(dev))
    out = (stats,) + tuple(t for t in (e, img) if t is not None)
    return out if len(out) > 1 else stats


def eval_stats(t):
    """The one read-back of flow_eval: its statistics tensor -> a dict of struct dflow_eval_stats's fields plus mean_epe
    = sum_err / n, outliers_pct = n_out_abs * 100 / n (the reference's two numbers) and kitti_fl_pct = n_out_kitti * 100 / n;
    the three are NaN when n == 0."""
    d = _struct_dict(_lib.EvalStats, t)
    d["mean_epe"] = d["sum_err"] / d["n"] if d["n"] else float("nan")
    d["outliers_pct"], d["kitti_fl_pct"] = _pct(d["n_out_abs"], d["n"]), _pct(d["n_out_kitti"], d["n"])
    return d


def flow_color(flow, max_flow=None, return_radius=False):
    """The Middlebury colour-wheel picture of a flow on the GPU (dflow_flow_color, DESIGN.md "Flow pictures and the warp
    check"): hue = direction, saturation = length over the radius.  flow is (H,W,3) float32 [U,V,valid] or (H,W,2) float32
    [dy,dx]; the last dimension says which.  Device tensor or host array; host data is uploaded to the current device.
    max_flow: the radius at which the colours saturate; None or 0: the largest flow of the field (found on the device,
    nothing is read back).  Returns the (H,W,3) uint8 picture in BGR order, black where the flow is unknown (not valid, not
    finite, or beyond 1e9), and with return_radius=True also the radius used as a one-element float32 device tensor.  Runs on
    torch's current stream and does not wait for it."""
    flow = _check(flow, "flow_color", "flow", torch.float32, (None, None, (2, 3)))
    H, W, _ = flow.shape
    dev = _device_of(flow)
    flow, = _on(dev, flow)
    ws, ws_bytes = _lib.workspace("dflow_flow_color_workspace_bytes", H, W, dev)
    img = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    radius = _out(return_radius, 1, torch.float32, dev)
    _lib.call("dflow_flow_color", H, W, flow.data_ptr(), _layout(flow), 0.0 if max_flow is None else float(max_flow), img.data_ptr(),
              _ptr(radius), ws.data_ptr(), ws_bytes, _lib.stream(dev))
    return (img, radius) if return_radius else img


def warp_eval(img1, img2, flow, err_thresh=10.0, err_max=30.0, warped=False, err=False, image=False, stats=None):
    """A quality check that needs no ground truth (dflow_warp_eval, DESIGN.md "Flow pictures and the warp check"): img2
    sampled bilinearly at (x + U, y + V) and compared with img1, the mean absolute difference of the three channels per pixel.
    img1, img2: (H,W,3) uint8 BGR; flow: (H,W,3) float32 [U,V,valid] or (H,W,2) float32 [dy,dx].  Device tensors or host
    arrays; host data is uploaded to the current device.  err_thresh (grey levels; the share of pixels above it is reported)
    and err_max (where the error picture saturates) default to 10 and 30: this build's choices, no reference sets them.
    Returns the statistics as a device tensor (struct dflow_photo_stats as 6 int64 words; photo_stats reads it back), then,
    if asked for, warped: (H,W,3) uint8, the warped second image; err: (H,W) float32; image: (H,W,3) uint8, the jet picture
    of min(err, err_max) / err_max in BGR order.  All three are 0 / -1 / black where the flow is unknown or leaves the frame.
    stats: the tensor of an earlier call (or torch.zeros(6, int64)) to add this pair's values to, so that a batch is
    totalled on the device.  Runs on torch's current stream and does not wait for it."""
    flow = _check(flow, "warp_eval", "flow", torch.float32, (None, None, (2, 3)))
    H, W, _ = flow.shape
    img1 = _check(img1, "warp_eval", "img1: the images", torch.uint8, (H, W, 3))
    img2 = _check(img2, "warp_eval", "img2: the images", torch.uint8, (H, W, 3))
    dev = _device_of(flow, img1, img2)
    flow, img1, img2 = _on(dev, flow, img1, img2)
    stats, accumulate = _stats_arg(stats, 6, dev, "warp_eval")
    ws, ws_bytes = _lib.workspace("dflow_warp_eval_workspace_bytes", H, W, dev)
    wp, e, pic = _out(warped, (H, W, 3), torch.uint8, dev), _out(err, (H, W), torch.float32, dev), _out(image, (H, W, 3), torch.uint8, dev)
    _lib.call("dflow_warp_eval", H, W, img1.data_ptr(), img2.data_ptr(), flow.data_ptr(), _layout(flow), float(err_thresh),
              float(err_max), _lib.WARP_FLAG_ACCUMULATE if accumulate else 0, stats.data_ptr(), _ptr(wp), _ptr(e), _ptr(pic),
              ws.data_ptr(), ws_bytes, _lib.stream(dev))
    out = (stats,) + tuple(t for t in (wp, e, pic) if t is not None)
    return out if len(out) > 1 else stats


def photo_stats(t):
    """The one read-back of warp_eval: its statistics tensor -> a dict of struct dflow_photo_stats's fields plus mean_err =
    sum_err / n and above_pct = n_above * 100 / n; the two are NaN when n == 0 (no pixel's target is inside the frame)."""
    d = _struct_dict(_lib.PhotoStats, t)
    d["mean_err"] = d["sum_err"] / d["n"] if d["n"] else float("nan")
    d["above_pct"] = _pct(d["n_above"], d["n"])
    return d


def flow_advance(flow, negate=False, counts=False):
    """Carries every vector of a flow to the pixel it points at (dflow_flow_advance, DESIGN.md "Prior proposals"): the flow of
    t -> t+1 becomes a prior for t+1 -> t+2 (constant velocity), and with negate=True a prior for the backward pass (the inverse
    flow).  flow is (H,W,2) float32 [dy,dx] or (H,W,3) float32 [U,V,valid]; the last dimension says which.  Device tensor or
    host array; host data is uploaded to the current device.  Vectors are rounded to integers; where several land on one pixel
    the one from the smallest raster index stays; a pixel nothing lands on is invalid.  Returns the (H,W,3) float32 [U,V,valid]
    device tensor, what DiscreteFlow.prior_proposals takes, and with counts=True also the int32[3] device tensor {claimed
    targets, claimants that lost, sources that did not take part}.  Runs on torch's current stream and does not wait for it."""
    flow = _check(flow, "flow_advance", "flow", torch.float32, (None, None, (2, 3)))
    H, W, _ = flow.shape
    dev = _device_of(flow)
    flow, = _on(dev, flow)
    ws, ws_bytes = _lib.workspace("dflow_flow_advance_workspace_bytes", H, W, dev)
    out = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    cnt = _out(counts, 3, torch.int32, dev)
    _lib.call("dflow_flow_advance", H, W, flow.data_ptr(), _layout(flow), _lib.ADVANCE_NEGATE if negate else 0, out.data_ptr(),
              _ptr(cnt), ws.data_ptr(), ws_bytes, _lib.stream(dev))
    return (out, cnt) if counts else out


def pyr_down(img1, img2=None):
    """One level of an image pyramid (dflow_pyr_down, DESIGN.md "Coarse to fine"): a (H,W,3) uint8 BGR image, or the two images
    of a pair in one launch, smoothed with the 5x5 binomial kernel [1,4,6,4,1] x [1,4,6,4,1] / 256 (replicated border, integer
    arithmetic, one rounding) and sampled at the even pixels -> ((H+1)//2, (W+1)//2, 3) uint8 device tensor(s).  Device tensors or
    host arrays; host data is uploaded to the current device.  Returns the level of img1, or with img2 the pair of levels.  Runs
    on torch's current stream and does not wait for it."""
    img1 = _check(img1, "pyr_down", "img1", torch.uint8, (None, None, 3))
    H, W, _ = img1.shape
    imgs = [img1] if img2 is None else [img1, _check(img2, "pyr_down", "img2", torch.uint8, (H, W, 3))]
    dev = _device_of(*imgs)
    imgs = _on(dev, *imgs)
    outs = [torch.empty(((H + 1) // 2, (W + 1) // 2, 3), dtype=torch.uint8, device=dev) for _ in imgs]
    _lib.call("dflow_pyr_down", H, W, imgs[0].data_ptr(), _ptr(imgs[1] if img2 is not None else None), outs[0].data_ptr(),
              _ptr(outs[1] if img2 is not None else None), _lib.stream(dev))
    return outs[0] if img2 is None else tuple(outs)


def flow_upsample(flow, size, counts=False):
    """The flow of a pyramid level as a prior for the next finer one (dflow_flow_upsample, DESIGN.md "Coarse to fine"): flow is
    ((H+1)//2, (W+1)//2, 2) float32 [dy,dx] or (.., 3) float32 [U,V,valid] for size = (H, W); the last dimension says which.
    Device tensor or host array; host data is uploaded to the current device.  Coarse pixel j sits at fine position 2j; a fine
    pixel gets twice the mean of its four coarse corners where all four are valid and finite, else twice its corner (y>>1, x>>1),
    else it is invalid.  Returns the (H,W,3) float32 [U,V,valid] device tensor, what DiscreteFlow.prior_proposals takes, and with
    counts=True also the int32[3] device tensor {bilinear, nearest, invalid}.  Runs on torch's current stream and does not wait
    for it."""
    H, W = (int(v) for v in size)
    if H < 1 or W < 1:
        raise ValueError("flow_upsample: size must be (H, W) >= 1, got %r" % (size,))
    flow = _check(flow, "flow_upsample", "flow", torch.float32, ((H + 1) // 2, (W + 1) // 2, (2, 3)))
    dev = _device_of(flow)
    flow, = _on(dev, flow)
    out = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    cnt = _out(counts, 3, torch.int32, dev)
    _lib.call("dflow_flow_upsample", H, W, flow.data_ptr(), _layout(flow), out.data_ptr(), _ptr(cnt), _lib.stream(dev))
    return (out, cnt) if counts else out


def flow_consistency(fwd, bwd, thresh, bilinear=False, both=False, err=False, counts=False):
    """The forward/backward check in image coordinates (dflow_flow_consistency, DESIGN.md "Forward/backward check in image
    coordinates"): the forward vector at p is kept if the backward vector at p + f(p) undoes it to within thresh pixels
    (|f(p) + b(p + f(p))| <= thresh).  Not fb_consistency, which restates the reference's check with its transposed lookup.  fwd
    and bwd are (H,W,2) float32 [dy,dx] or (H,W,3) float32 [U,V,valid], each on its own; the last dimension says which.  Device
    tensors or host arrays; host data is uploaded to the current device.  The backward vector is looked up at the rounded
    target, or with bilinear=True interpolated from the four pixels around the exact one (the same result on integer flows).  A
    vector that is invalid or not finite, whose target leaves the frame or meets an invalid vector, or whose error is above
    thresh becomes [0,0,0].  Returns the (H,W,3) float32 [U,V,valid] device tensor of the forward field, or a tuple in the order
    (out_fwd[, out_bwd][, err_fwd[, err_bwd]][, counts]): both=True checks the backward field against the forward one in the same
    launch; err=True adds the (H,W) float32 error planes (-1 where no error was formed); counts=True adds the int32 device
    tensor {consistent, above, bwd_invalid, outside, fwd_invalid}, (5,) or with both (2,5), row 0 the forward field's.  Runs on
    torch's current stream and does not wait for it."""
    fwd = _check(fwd, "flow_consistency", "fwd", torch.float32, (None, None, (2, 3)))
    H, W, _ = fwd.shape
    bwd = _check(bwd, "flow_consistency", "bwd", torch.float32, (H, W, (2, 3)))
    thresh = float(thresh)
    if not (np.isfinite(thresh) and thresh >= 0):
        raise ValueError("flow_consistency: thresh must be finite and >= 0, got %r" % thresh)
    dev = _device_of(fwd, bwd)
    fwd, bwd = _on(dev, fwd, bwd)
    outs = [torch.empty((H, W, 3), dtype=torch.float32, device=dev), _out(both, (H, W, 3), torch.float32, dev)]
    errs = [_out(err, (H, W), torch.float32, dev), _out(err and both, (H, W), torch.float32, dev)]
    cnt = _out(counts, (2, 5) if both else (5,), torch.int32, dev)
    _lib.call("dflow_flow_consistency", H, W, fwd.data_ptr(), _layout(fwd), bwd.data_ptr(), _layout(bwd), thresh,
              _lib.FBC_BILINEAR if bilinear else 0, outs[0].data_ptr(), _ptr(outs[1]), _ptr(errs[0]), _ptr(errs[1]), _ptr(cnt),
              _lib.stream(dev))
    ret = tuple(t for t in outs + errs + [cnt] if t is not None)
    return ret if len(ret) > 1 else ret[0]


def segment_filter(flow, thresh, min_size, keep_singletons=False, segments=False, sizes=False, counts=False):
    """The small-segment filter of a sparse flow field (dflow_segment_filter, DESIGN.md "Small-segment filter"): the good vectors
    (valid and finite) fall into segments, the connected components under "4-adjacent and |dU| + |dV| <= thresh", and every
    segment of fewer than min_size pixels is removed.  Not compat.remove_small_segments, which restates the reference's
    sequential flood fill on the host.  flow is (H,W,2) float32 [dy,dx] or (H,W,3) float32 [U,V,valid]; the last dimension says
    which.  Device tensor or host array; host data is uploaded to the current device.  keep_singletons=True keeps segments of
    one pixel whatever min_size is.  Returns the (H,W,3) float32 [U,V,valid] device tensor, removed and invalid pixels [0,0,0],
    or a tuple in the order (out[, segment][, size][, counts]): segments=True adds the (H,W) int32 plane of segment ids (the
    smallest raster index of the segment, -1 where there is no vector), sizes=True the (H,W) int32 plane of segment sizes (0
    there), both of the input's segments; counts=True the int32[4] device tensor {segments, segments removed, members, pixels
    removed}.  Runs on torch's current stream and does not wait for it."""
    flow = _check(flow, "segment_filter", "flow", torch.float32, (None, None, (2, 3)))
    H, W, _ = flow.shape
    thresh = float(thresh)
    if not (np.isfinite(thresh) and thresh >= 0):
        raise ValueError("segment_filter: thresh must be finite and >= 0, got %r" % thresh)
    if not (isinstance(min_size, (int, np.integer)) and 0 <= min_size < 2 ** 31):
        raise ValueError("segment_filter: min_size must be an int in [0, 2^31), got %r" % (min_size,))
    dev = _device_of(flow)
    flow, = _on(dev, flow)
    ws, ws_bytes = _lib.workspace("dflow_segment_filter_workspace_bytes", H, W, dev)
    out = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    extra = [_out(segments, (H, W), torch.int32, dev), _out(sizes, (H, W), torch.int32, dev), _out(counts, 4, torch.int32, dev)]
    _lib.call("dflow_segment_filter", H, W, flow.data_ptr(), _layout(flow), thresh, int(min_size),
              _lib.SEG_KEEP_SINGLETONS if keep_singletons else 0, out.data_ptr(), _ptr(extra[0]), _ptr(extra[1]), _ptr(extra[2]),
              ws.data_ptr(), ws_bytes, _lib.stream(dev))
    ret = tuple(t for t in [out] + extra if t is not None)
    return ret if len(ret) > 1 else ret[0]


FRAME_INTERP_COUNTS = ("from1", "from2", "filled", "unknown", "blended", "one_sided", "fallback", "lost")


def _frame_interp_gate(fn, img1, img2, fwd, bwd, fill_rounds, occl_thresh):
    """The inputs of frame_interp / frame_sequence through the input gate, on one device: (H, W, dev, img1, img2, fwd, bwd)."""
    fwd = _check(fwd, fn, "fwd", torch.float32, (None, None, (2, 3)))
    H, W, _ = fwd.shape
    img1 = _check(img1, fn, "img1: the images", torch.uint8, (H, W, 3))
    img2 = _check(img2, fn, "img2: the images", torch.uint8, (H, W, 3))
    if bwd is not None:
        bwd = _check(bwd, fn, "bwd", torch.float32, (H, W, (2, 3)))
    if not (isinstance(fill_rounds, (int, np.integer)) and 0 <= fill_rounds <= 64):
        raise ValueError("%s: fill_rounds must be an int in [0, 64], got %r" % (fn, fill_rounds))
    if not (np.isfinite(occl_thresh) and occl_thresh >= 0):
        raise ValueError("%s: occl_thresh must be finite and >= 0, got %r" % (fn, occl_thresh))
    dev = _device_of(fwd, img1, img2, *([bwd] if bwd is not None else []))
    ts = _on(dev, *([img1, img2, fwd] + ([bwd] if bwd is not None else [])))
    return H, W, dev, ts[0], ts[1], ts[2], ts[3] if bwd is not None else None


def _frame_interp_call(H, W, dev, img1, img2, fwd, bwd, t, fill_rounds, occl_thresh, planes, want_source, want_counts):
    """One dflow_frame_interp into new outputs, with the scratch planes (keys, motion, motion_tmp) of the caller."""
    keys, mot, tmp = planes
    out = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    src, cnt = _out(want_source, (H, W), torch.uint8, dev), _out(want_counts, 8, torch.int32, dev)
    _lib.call("dflow_frame_interp", H, W, img1.data_ptr(), img2.data_ptr(), fwd.data_ptr(), _layout(fwd), _ptr(bwd),
              _layout(bwd) if bwd is not None else 0, _frame_time(t), int(fill_rounds), float(occl_thresh), 0, out.data_ptr(), keys.data_ptr(),
              mot.data_ptr(), _ptr(tmp), _ptr(src), _ptr(cnt), _lib.stream(dev))
    return out, src, cnt


def _frame_time(t):
    """t as the float32 the library receives; ValueError unless that lies in (0, 1)."""
    t = float(np.float32(t))
    if not (np.isfinite(t) and 0.0 < t < 1.0):
        raise ValueError("frame_interp: t must lie in (0, 1) as a float32, got %r" % (t,))
    return t


def _frame_interp_planes(H, W, dev, fill_rounds):
    return (torch.empty((H, W), dtype=torch.int64, device=dev), torch.empty((H, W, 3), dtype=torch.float32, device=dev),
            _out(fill_rounds > 0, (H, W, 3), torch.float32, dev))


def frame_interp(img1, img2, fwd, bwd=None, t=0.5, fill_rounds=8, occl_thresh=30.0, motion=False, source=False, counts=False):
    """The frame at time t, 0 < t < 1, between img1 (time 0) and img2 (time 1) (dflow_frame_interp, DESIGN.md "Frame
    interpolation"): every pixel of img1 is carried t of the way along its forward vector, with bwd every pixel of img2 1 - t
    of the way along its backward vector; where several land on one pixel the one whose two ends look most alike stays;
    pixels nothing lands on take a neighbour's motion in up to fill_rounds rounds; then both frames are sampled along each
    pixel's motion and blended s*c1 + t*c2, or, where the two samples differ by more than occl_thresh grey levels, only the
    frame the motion came from is used.  A pixel without a motion is the plain blend of the two frames.  img1, img2: (H,W,3)
    uint8 BGR; fwd, bwd: (H,W,2) float32 [dy,dx] or (H,W,3) float32 [U,V,valid], each on its own; the last dimension says
    which.  Device tensors or host arrays; host data is uploaded to the current device.  Returns the (H,W,3) uint8 device
    tensor, or a tuple in the order (frame[, motion][, source][, counts]): motion=True adds the (H,W,3) float32 field [mU, mV,
    known] after the fill, source=True the (H,W) uint8 plane 0 none / 1 from img1 / 2 from img2 / 3 filled, counts=True the
    int32[8] device tensor FRAME_INTERP_COUNTS.  Runs on torch's current stream and does not wait for it."""
    _frame_time(t)
    H, W, dev, img1, img2, fwd, bwd = _frame_interp_gate("frame_interp", img1, img2, fwd, bwd, fill_rounds, occl_thresh)
    planes = _frame_interp_planes(H, W, dev, fill_rounds)
    out, src, cnt = _frame_interp_call(H, W, dev, img1, img2, fwd, bwd, t, fill_rounds, occl_thresh, planes, source, counts)
    ret = tuple(x for x in (out, planes[1] if motion else None, src, cnt) if x is not None)
    return ret if len(ret) > 1 else out


def frame_sequence(img1, img2, fwd, bwd=None, n=1, fill_rounds=8, occl_thresh=30.0, counts=False):
    """The n frames at t = k / (n + 1), k = 1..n, between img1 and img2: n calls of dflow_frame_interp that share one set of
    scratch planes (t is rounded to float32 once, as frame_interp does, so every frame equals that of a single call).
    Arguments as frame_interp.  Returns the list of (H,W,3) uint8 device tensors, with counts=True the pair (frames, list of
    int32[8] device tensors).  Runs on torch's current stream and does not wait for it."""
    if not (isinstance(n, (int, np.integer)) and 1 <= n <= 1024):
        raise ValueError("frame_sequence: n must be an int in [1, 1024], got %r" % (n,))
    H, W, dev, img1, img2, fwd, bwd = _frame_interp_gate("frame_sequence", img1, img2, fwd, bwd, fill_rounds, occl_thresh)
    planes = _frame_interp_planes(H, W, dev, fill_rounds)
    frames, cnts = [], []
    for k in range(1, n + 1):
        out, _, cnt = _frame_interp_call(H, W, dev, img1, img2, fwd, bwd, k / (n + 1), fill_rounds, occl_thresh, planes, False, counts)
        frames.append(out)
        cnts.append(cnt)
    return (frames, cnts) if counts else frames


FLOW_WMEDIAN_COUNTS = ("good", "valid", "filled", "altered")
WMEDIAN_NCOLOR = 766                    # |db| + |dg| + |dr| = 0 .. 765
_wmedian_uploaded = {}                  # (device, radius, bytes of space, bytes of colour) -> the two device tensors


def wmedian_tables(radius, sigma_space=None, sigma_color=None):
    """The weight tables of flow_wmedian as (space, color), each a numpy uint8 array or None for a None sigma (all ones), computed
    in float64: space[|dy|,|dx|] = floor(255 exp(-(dy^2 + dx^2) / (2 sigma_space^2)) + 0.5), (radius+1, radius+1);
    color[d] = floor(255 exp(-d / (3 sigma_color)) + 0.5), d = |db| + |dg| + |dr| = 0..765 (sigma_color is in grey levels per
    channel).  ValueError for a radius outside 1..8 or a sigma that is not finite or not positive."""
    if not (isinstance(radius, (int, np.integer)) and 1 <= radius <= 8):
        raise ValueError("wmedian_tables: radius must be an int in [1, 8], got %r" % (radius,))
    for name, s in (("sigma_space", sigma_space), ("sigma_color", sigma_color)):
        if s is not None and not (isinstance(s, (int, float, np.integer, np.floating)) and np.isfinite(s) and s > 0):
            raise ValueError("wmedian_tables: %s must be finite and > 0, got %r" % (name, s))
    space = color = None
    if sigma_space is not None:
        d2 = np.arange(radius + 1, dtype=np.float64) ** 2
        space = np.floor(255.0 * np.exp(-(d2[:, None] + d2[None, :]) / (2.0 * float(sigma_space) ** 2)) + 0.5).astype(np.uint8)
    if sigma_color is not None:
        color = np.floor(255.0 * np.exp(-np.arange(WMEDIAN_NCOLOR, dtype=np.float64) / (3.0 * float(sigma_color))) + 0.5).astype(np.uint8)
    return space, color


def _wmedian_tables_arg(radius, tables, guided):
    """tables=(space, color) checked -> contiguous uint8 arrays or None; an unguided call drops the colour table."""
    if not (isinstance(tables, (tuple, list)) and len(tables) == 2):
        raise ValueError("flow_wmedian: tables must be the pair (space, color), got %r" % (tables,))
    out = []
    for name, t, n in (("space", tables[0], (radius + 1) ** 2), ("color", tables[1], WMEDIAN_NCOLOR)):
        if t is not None:
            t = np.ascontiguousarray(t)
            if t.dtype != np.uint8 or t.size != n:
                raise ValueError("flow_wmedian: the %s table must be uint8 with %d entries, got %s %s" % (name, n, t.shape, t.dtype))
        out.append(t)
    if guided and out[1] is None:
        out[1] = np.ones(WMEDIAN_NCOLOR, np.uint8)
    return out[0], out[1] if guided else None


def flow_wmedian(flow, img=None, radius=3, sigma_space=None, sigma_color=10.0, iterations=1, keep_holes=False, reject=None,
                 counts=False, tables=None):
    """The edge-aware weighted median filter of a flow field (dflow_flow_wmedian, DESIGN.md "Weighted median filter"): every
    pixel gets, per component, the lower weighted median of the good vectors in the (2 radius + 1)^2 window around it, the
    weight of a neighbour being space[|dy|,|dx|] * color[colour distance to the pixel in img] (wmedian_tables).  Holes are
    filled from their windows.  flow is (H,W,2) float32 [dy,dx] or (H,W,3) float32 [U,V,valid]; img the (H,W,3) uint8 BGR guide
    or None (unguided: sigma_color is ignored).  Device tensors or host arrays; host data is uploaded to the current device.
    sigma_space=None weighs every distance alike; tables=(space, color) overrides both sigmas.  iterations (1..16) passes
    ping-pong between two buffers.  keep_holes=True leaves a pixel without a good vector [0,0,0].  reject=T filters nothing:
    a good vector stays bit for bit if |U - mU| + |V - mV| <= T and becomes [0,0,0] otherwise (one pass only).  Returns the
    (H,W,3) float32 [U,V,valid] device tensor, with counts=True the pair (out, int32[4] device tensor FLOW_WMEDIAN_COUNTS of
    the last pass).  Uploaded tables are kept per device and parameter set.  Runs on torch's current stream and does not wait
    for it."""
    flow = _check(flow, "flow_wmedian", "flow", torch.float32, (None, None, (2, 3)))
    H, W, _ = flow.shape
    guided = img is not None
    if guided:
        img = _check(img, "flow_wmedian", "img", torch.uint8, (H, W, 3))
    if not (isinstance(radius, (int, np.integer)) and 1 <= radius <= 8):
        raise ValueError("flow_wmedian: radius must be an int in [1, 8], got %r" % (radius,))
    if not (isinstance(iterations, (int, np.integer)) and 1 <= iterations <= 16):
        raise ValueError("flow_wmedian: iterations must be an int in [1, 16], got %r" % (iterations,))
    flags, thresh = _lib.WMED_KEEP_HOLES if keep_holes else 0, 0.0
    if reject is not None:
        thresh = float(reject)
        if not (np.isfinite(thresh) and thresh >= 0):
            raise ValueError("flow_wmedian: reject must be finite and >= 0, got %r" % (reject,))
        if iterations > 1:
            raise ValueError("flow_wmedian: reject cannot be combined with iterations > 1")
        flags |= _lib.WMED_REJECT
    if tables is None:
        tables = wmedian_tables(int(radius), sigma_space, sigma_color if guided else None)
    space, color = _wmedian_tables_arg(int(radius), tables, guided)
    dev = _device_of(flow, *([img] if guided else []))
    ts = _on(dev, flow, *([img] if guided else []))
    flow, img = ts[0], ts[1] if guided else None
    key = (dev, int(radius), None if space is None else space.tobytes(), None if color is None else color.tobytes())
    if key not in _wmedian_uploaded:
        _wmedian_uploaded[key] = tuple(None if t is None else torch.from_numpy(t.reshape(-1)).to(dev) for t in (space, color))
    dspace, dcolor = _wmedian_uploaded[key]
    cnt = _out(counts, 4, torch.int32, dev)
    bufs = [torch.empty((H, W, 3), dtype=torch.float32, device=dev) for _ in range(min(int(iterations), 2))]
    src = flow
    for it in range(int(iterations)):
        out = bufs[it & 1]
        _lib.call("dflow_flow_wmedian", H, W, src.data_ptr(), _layout(src), _ptr(img), int(radius), _ptr(dspace), _ptr(dcolor), thresh,
                  flags, out.data_ptr(), _ptr(cnt), _lib.stream(dev))
        src = out
    return (src, cnt) if counts else src


def flow_gate(flow, score, lo=float("-inf"), hi=float("inf"), counts=False):
    """The gate of a flow field by a score plane (dflow_flow_gate, DESIGN.md "Label confidence"): a good vector (valid and finite)
    whose score lies in [lo, hi] stays bit for bit, every other pixel becomes [0,0,0]; a NaN score fails.  flow is (H,W,2) float32
    [dy,dx] or (H,W,3) float32 [U,V,valid], the last dimension says which; score is (H,W) float32, the margin of
    DiscreteFlow.confidence or any other plane (the err plane of flow_consistency with hi=T).  Device tensors or host arrays; host
    data is uploaded to the current device.  lo and hi may be infinite, not NaN, lo <= hi.  Returns the (H,W,3) float32 [U,V,valid]
    device tensor, with counts=True the pair (out, int32[2] device tensor {good, kept}).  The input is not modified.  Runs on
    torch's current stream and does not wait for it."""
    flow = _check(flow, "flow_gate", "flow", torch.float32, (None, None, (2, 3)))
    H, W, _ = flow.shape
    score = _check(score, "flow_gate", "score", torch.float32, (H, W))
    for name, v in (("lo", lo), ("hi", hi)):
        if not isinstance(v, (int, float, np.integer, np.floating)) or np.isnan(np.float32(v)):
            raise ValueError("flow_gate: %s must be a number, not NaN, got %r" % (name, v))
    lo, hi = float(np.float32(lo)), float(np.float32(hi))
    if lo > hi:
        raise ValueError("flow_gate: lo=%g is above hi=%g" % (lo, hi))
    dev = _device_of(flow, score)
    flow, score = _on(dev, flow, score)
    out = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    cnt = _out(counts, 2, torch.int32, dev)
    _lib.call("dflow_flow_gate", H, W, flow.data_ptr(), _layout(flow), score.data_ptr(), lo, hi, out.data_ptr(), _ptr(cnt), _lib.stream(dev))
    return (out, cnt) if counts else out


MOTION_MODELS = {"affine": _lib.MOTION_AFFINE, "homography": _lib.MOTION_HOMOGRAPHY}
MOTION_FIT_COUNTS = ("scored", "inliers", "degenerate", "best_round", "best_j", "best_count", "accepted", "skipped")


def _motion_fit_gate(fn, flow, model, thresh, n_hyp, lo_rounds, polish, step, seed, exclude):
    """The arguments of motion_fit / motion_layers through the input gate, before any device is touched: (flow, exclude)."""
    flow = _check(flow, fn, "flow", torch.float32, (None, None, (2, 3)))
    H, W, _ = flow.shape
    if exclude is not None:
        exclude = _check(exclude, fn, "exclude", torch.uint8, (H, W))
    if model not in MOTION_MODELS:
        raise ValueError("%s: model must be 'affine' or 'homography', got %r" % (fn, model))
    if not (isinstance(thresh, (int, float, np.integer, np.floating)) and np.isfinite(np.float32(thresh)) and np.float32(thresh) > 0):
        raise ValueError("%s: thresh must be finite and > 0 as a float32, got %r" % (fn, thresh))
    for name, v, lo, hi in (("n_hyp", n_hyp, 1, 65536), ("lo_rounds", lo_rounds, 0, 4), ("polish", polish, 0, 4), ("step", step, 1, 64),
                            ("seed", seed, 0, 2 ** 64 - 1)):
        if not (isinstance(v, (int, np.integer)) and lo <= v <= hi):
            raise ValueError("%s: %s must be an int in [%d, %d], got %r" % (fn, name, lo, hi, v))
    return flow, exclude


def _motion_fit_call(flow, exclude, model, thresh, n_hyp, lo_rounds, polish, step, seed, scratch, classes, model_flow, residual, counts):
    """One dflow_motion_fit on device tensors with the caller's scratch planes (models, hyp_counts, state) into new outputs."""
    H, W, _ = flow.shape
    dev = flow.device
    models, hyp_counts, state = scratch
    out = torch.empty(9, dtype=torch.float32, device=dev)
    extra = [_out(classes, (H, W), torch.uint8, dev), _out(model_flow, (H, W, 3), torch.float32, dev),
             _out(residual, (H, W, 3), torch.float32, dev), _out(counts, 8, torch.int32, dev)]
    _lib.call("dflow_motion_fit", H, W, flow.data_ptr(), _layout(flow), _ptr(exclude), MOTION_MODELS[model], float(thresh), int(n_hyp),
              int(lo_rounds), int(polish), int(step), int(seed), 0, out.data_ptr(), models.data_ptr(), hyp_counts.data_ptr(),
              state.data_ptr(), _ptr(extra[0]), _ptr(extra[1]), _ptr(extra[2]), _ptr(extra[3]), _lib.stream(dev))
    return out.view(3, 3), extra


def _motion_fit_scratch(n_hyp, dev):
    return (torch.empty(int(n_hyp) * 9, dtype=torch.float32, device=dev), torch.empty(int(n_hyp), dtype=torch.int32, device=dev),
            torch.empty(32, dtype=torch.int64, device=dev))


def motion_fit(flow, model="affine", thresh=1.0, n_hyp=1024, lo_rounds=1, polish=2, step=1, seed=0, exclude=None, classes=False,
               model_flow=False, residual=False, counts=False):
    """The dominant motion of a flow field (dflow_motion_fit, DESIGN.md "Global-motion fit"): the affine map or the homography
    M: (x,y,1) -> (X,Y,W), position in the second frame (X/W, Y/W), that most vectors agree with to within thresh pixels, found
    from n_hyp random minimal samples per round, lo_rounds further rounds sampled among the best model's inliers and, for an
    affine map, `polish` least-squares steps.  flow is (H,W,2) float32 [dy,dx] or (H,W,3) float32 [U,V,valid]; exclude an (H,W)
    uint8 mask, non-zero = the pixel takes no part, or None.  Device tensors or host arrays; host data is uploaded to the current
    device.  step > 1 scores only every step-th row and column.  Returns the (3,3) float32 device tensor, the identity when no
    model was found, or a tuple in the order (model[, classes][, model_flow][, residual][, counts]): classes=True adds the (H,W)
    uint8 plane 0 no vector / 1 inlier / 2 outlier / 3 excluded, model_flow=True the model's own (H,W,3) [U,V,valid] flow (a
    prior for DiscreteFlow.front_end), residual=True the (H,W,3) flow minus the model's, counts=True the int32[8] device tensor
    MOTION_FIT_COUNTS.  Runs on torch's current stream and does not wait for it."""
    flow, exclude = _motion_fit_gate("motion_fit", flow, model, thresh, n_hyp, lo_rounds, polish, step, seed, exclude)
    dev = _device_of(flow, *([exclude] if exclude is not None else []))
    ts = _on(dev, flow, *([exclude] if exclude is not None else []))
    out, extra = _motion_fit_call(ts[0], ts[1] if exclude is not None else None, model, thresh, n_hyp, lo_rounds, polish, step, seed,
                                  _motion_fit_scratch(n_hyp, dev), classes, model_flow, residual, counts)
    ret = tuple(t for t in [out] + extra if t is not None)
    return ret if len(ret) > 1 else out


def motion_layers(flow, k, exclude=None, **fit_args):
    """k successive motion fits of one flow field: the inliers of each fit are excluded from the fits after it, on the device,
    with nothing read back in between.  fit_args are motion_fit's (model, thresh, n_hyp, lo_rounds, polish, step, seed).  Returns
    (models, layers): the list of k (3,3) float32 device tensors and the (H,W) uint8 device plane, 0 = no layer, i = inlier of
    fit i (1-based).  Runs on torch's current stream and does not wait for it."""
    if not (isinstance(k, (int, np.integer)) and 1 <= k <= 255):
        raise ValueError("motion_layers: k must be an int in [1, 255], got %r" % (k,))
    unknown = set(fit_args) - {"model", "thresh", "n_hyp", "lo_rounds", "polish", "step", "seed"}
    if unknown:
        raise ValueError("motion_layers: unknown arguments %s" % sorted(unknown))
    args = dict(dict(model="affine", thresh=1.0, n_hyp=1024, lo_rounds=1, polish=2, step=1, seed=0), **fit_args)
    flow, exclude = _motion_fit_gate("motion_layers", flow, exclude=exclude, **args)
    dev = _device_of(flow, *([exclude] if exclude is not None else []))
    flow, = _on(dev, flow)
    H, W, _ = flow.shape
    taken = (_on(dev, exclude)[0] != 0).to(torch.uint8) if exclude is not None else torch.zeros((H, W), dtype=torch.uint8, device=dev)
    layers = torch.zeros((H, W), dtype=torch.uint8, device=dev)
    scratch = _motion_fit_scratch(args["n_hyp"], dev)
    models = []
    for i in range(1, int(k) + 1):
        m, extra = _motion_fit_call(flow, taken, scratch=scratch, classes=True, model_flow=False, residual=False, counts=False, **args)
        inl = extra[0] == 1
        layers[inl] = i
        taken = taken | inl.to(torch.uint8)
        models.append(m)
    return models, layers


# ---------------------------------------------------------------------- epipolar geometry (csrc/epipolar.hip)
EPIPOLAR_FIT_COUNTS = ("scored", "inliers", "degenerate", "best_round", "best_slot", "best_count", "models_per_1000", "reserved")


def epipolar_fit(flow, thresh=1.0, n_hyp=512, lo_rounds=1, step=1, seed=0, exclude=None, classes=False, residual=False, counts=False):
    """The epipolar geometry of a flow field (dflow_epipolar_fit, DESIGN.md "Epipolar-geometry fit"): the fundamental matrix
    that most vectors agree with to within a Sampson distance of thresh pixels, found from n_hyp random 7-point samples per
    round (each gives up to three models) and lo_rounds further rounds sampled among the best model's inliers.  The model of a
    camera moving through a rigid scene with depth; motion_fit's homography fits one plane of it.  flow is (H,W,2) float32
    [dy,dx] or (H,W,3) float32 [U,V,valid]; exclude an (H,W) uint8 mask, non-zero = the pixel takes no part, or None.  Device
    tensors or host arrays; host data is uploaded to the current device.  step > 1 scores only every step-th row and column.
    Returns the (3,3) float32 device tensor F^ in the centred, scaled coordinates the header defines (epipolar_geometry turns it
    into pixels), all zeros when no model was found (a still camera, a line of pixels, fewer than 7 vectors), or a tuple in the
    order (model[, classes][, residual][, counts]): classes=True adds the (H,W) uint8 plane 0 no vector / 1 inlier / 2 outlier /
    3 excluded, residual=True the (H,W) float32 Sampson distance in pixels (-1 where there is no vector), counts=True the
    int32[8] device tensor EPIPOLAR_FIT_COUNTS.  Runs on torch's current stream and does not wait for it."""
    fn = "epipolar_fit"
    flow = _check(flow, fn, "flow", torch.float32, (None, None, (2, 3)))
    H, W, _ = flow.shape
    if exclude is not None:
        exclude = _check(exclude, fn, "exclude", torch.uint8, (H, W))
    if not (isinstance(thresh, (int, float, np.integer, np.floating)) and np.isfinite(np.float32(thresh)) and np.float32(thresh) > 0):
        raise ValueError("%s: thresh must be finite and > 0 as a float32, got %r" % (fn, thresh))
    for name, v, lo, hi in (("n_hyp", n_hyp, 1, _lib.EPIPOLAR_MAX_HYP), ("lo_rounds", lo_rounds, 0, 4), ("step", step, 1, 64),
                            ("seed", seed, 0, 2 ** 64 - 1)):
        if not (isinstance(v, (int, np.integer)) and lo <= v <= hi):
            raise ValueError("%s: %s must be an int in [%d, %d], got %r" % (fn, name, lo, hi, v))
    dev = _device_of(flow, *([exclude] if exclude is not None else []))
    ts = _on(dev, flow, *([exclude] if exclude is not None else []))
    flow, exclude = ts[0], ts[1] if exclude is not None else None
    out = torch.empty(9, dtype=torch.float32, device=dev)
    models = torch.empty(3 * int(n_hyp) * 9, dtype=torch.float32, device=dev)
    hyp_counts = torch.empty(3 * int(n_hyp), dtype=torch.int32, device=dev)
    state = torch.empty(32, dtype=torch.int64, device=dev)
    extra = [_out(classes, (H, W), torch.uint8, dev), _out(residual, (H, W), torch.float32, dev), _out(counts, 8, torch.int32, dev)]
    _lib.call("dflow_epipolar_fit", H, W, flow.data_ptr(), _layout(flow), _ptr(exclude), float(thresh), int(n_hyp), int(lo_rounds),
              int(step), int(seed), 0, out.data_ptr(), models.data_ptr(), hyp_counts.data_ptr(), state.data_ptr(), _ptr(extra[0]),
              _ptr(extra[1]), _ptr(extra[2]), _lib.stream(dev))
    ret = tuple(t for t in [out.view(3, 3)] + extra if t is not None)
    return ret if len(ret) > 1 else ret[0]


def epipolar_geometry(model, h, w):
    """What the nine numbers of epipolar_fit mean in pixels, in host float64, after the caller has read them (model: anything
    np.asarray takes, 9 values).  Returns a dict: F, the (3,3) fundamental matrix in pixel coordinates, T^T F^ T with the header's
    T, so that (x',y',1) F (x,y,1)^T = 0; e1, the epipole in frame 1 (F e1 = 0), and e2, the epipole in frame 2 (F^T e2 = 0), as
    homogeneous 3-vectors, each the cross product of the two rows (for e2: columns) of F whose product is longest; foe, e1 in
    pixels (x, y), the focus of expansion when the camera moves forward, or None when e1 lies at infinity (a sideways motion)
    or there is no model."""
    m = np.asarray(model, np.float64).reshape(3, 3)
    if not (isinstance(h, (int, np.integer)) and isinstance(w, (int, np.integer)) and 1 <= h <= 8192 and 1 <= w <= 8192):
        raise ValueError("epipolar_geometry: h and w must be ints in [1, 8192], got %r, %r" % (h, w))
    P = 1.0
    while P < max(h, w):
        P *= 2.0
    s, cx, cy = 1.0 / P, (w - 1) * 0.5, (h - 1) * 0.5
    T = np.array([[s, 0.0, -cx * s], [0.0, s, -cy * s], [0.0, 0.0, 1.0]])
    F = T.T @ m @ T

    def null(rows):
        products = [np.cross(rows[i], rows[j]) for i, j in ((0, 1), (0, 2), (1, 2))]
        return max(products, key=lambda c: float(c @ c))
    e1, e2 = null(F), null(F.T)
    scale = float(np.abs(e1).max())
    foe = (float(e1[0] / e1[2]), float(e1[1] / e1[2])) if scale > 0.0 and abs(e1[2]) > 1e-12 * scale else None
    return dict(F=F, e1=e1, e2=e2, foe=foe)


# ---------------------------------------------------------------------- two-view reconstruction (csrc/two_view.hip)
TWO_VIEW_COUNTS = ("voters", "votes", "runner_up", "candidate", "front", "behind", "flat", "reserved")


def _finite(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and np.isfinite(v)


def two_view_intrinsics(fn, H, W, focal, center):
    """(fx, fy, cx, cy) as Python floats: focal a number or a pair, None = max(H, W), synth's camera; center a pair (cx, cy), None
    = the frame's centre.  ValueError for anything else."""
    if focal is None:
        focal = float(max(H, W))
    pair = tuple(focal) if isinstance(focal, (tuple, list)) else (focal, focal)
    if len(pair) != 2 or not all(_finite(v) and v > 0 for v in pair):
        raise ValueError("%s: focal must be a finite number > 0 or a pair of them, got %r" % (fn, focal))
    if center is None:
        center = ((W - 1) * 0.5, (H - 1) * 0.5)
    if not (isinstance(center, (tuple, list)) and len(center) == 2 and all(_finite(v) for v in center)):
        raise ValueError("%s: center must be a pair of finite numbers (cx, cy), got %r" % (fn, center))
    return float(pair[0]), float(pair[1]), float(center[0]), float(center[1])


def two_view(flow, model, focal=None, center=None, part=None, step=1, depth=False, classes=False, err=False, counts=False):
    """The camera motion and the depths a flow field and its fundamental matrix imply (dflow_two_view, DESIGN.md "Two-view
    reconstruction").  flow is (H,W,2) float32 [dy,dx] or (H,W,3) float32 [U,V,valid]; model the (3,3) or (9,) float32 F^ of
    epipolar_fit, on the device or on the host (it is not read here); focal a number or a pair (fx, fy) in pixels, None =
    max(H, W), synth's camera; center the principal point (cx, cy), None = the frame's centre; part an (H,W) uint8 plane, a
    pixel votes iff its byte is 1 (epipolar_fit's classes), or None = every vector; step > 1 lets only every step-th row and
    column vote.  Returns the float64[16] device tensor {R row-major, t, 1, sigma2/sigma1, sigma3/sigma1, candidate}, all zeros
    with [15] = -1 when there is no pose (two_view_pose reads it on the host), or a tuple in the order (pose[, depth][,
    classes][, err][, counts]): depth=True adds the (H,W) float32 depth in camera 1 in units of the baseline (0 without a
    vector or without parallax), classes=True the (H,W) uint8 plane 0 no vector / 1 in front of both cameras / 2 behind one / 3
    no parallax or no pose, err=True the (H,W) float32 reprojection error in pixels (-1 without a vector, +Inf where there is
    none), counts=True the int32[8] device tensor TWO_VIEW_COUNTS.  Runs on torch's current stream and does not wait for it."""
    fn = "two_view"
    flow = _check(flow, fn, "flow", torch.float32, (None, None, (2, 3)))
    H, W, _ = flow.shape
    m = model if isinstance(model, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(model))
    if m.dtype != torch.float32 or tuple(m.shape) not in ((3, 3), (9,)):
        raise ValueError("%s: model must be float32 (3,3) or (9,), got %s %s" % (fn, tuple(m.shape), m.dtype))
    if part is not None:
        part = _check(part, fn, "part", torch.uint8, (H, W))
    fx, fy, cx, cy = two_view_intrinsics(fn, H, W, focal, center)
    step = _int_in(fn, "step", step, 1, 64)
    given = [flow, m] + ([part] if part is not None else [])
    dev = _device_of(*given)
    ts = _on(dev, *given)
    flow, m, part = ts[0], ts[1], ts[2] if part is not None else None
    pose = torch.empty(16, dtype=torch.float64, device=dev)
    state = torch.empty(32, dtype=torch.int64, device=dev)
    extra = [_out(depth, (H, W), torch.float32, dev), _out(classes, (H, W), torch.uint8, dev), _out(err, (H, W), torch.float32, dev),
             _out(counts, 8, torch.int32, dev)]
    _lib.call("dflow_two_view", H, W, flow.data_ptr(), _layout(flow), m.data_ptr(), _ptr(part), fx, fy, cx, cy, step, 0, pose.data_ptr(),
              state.data_ptr(), _ptr(extra[0]), _ptr(extra[1]), _ptr(extra[2]), _ptr(extra[3]), _lib.stream(dev))
    ret = tuple(t for t in [pose] + extra if t is not None)
    return ret if len(ret) > 1 else ret[0]


def two_view_pose(pose):
    """What the 16 numbers of two_view mean, in host float64, after the caller has read them.  Returns a dict: R (3,3), t (3,),
    angle_deg and axis, the rotation's angle in [0, 180] and its unit axis (None for no rotation), singular (3,), the singular
    values of the essential matrix over the largest, candidate (int, -1: no pose; then R and t are zeros)."""
    p = np.asarray(pose, np.float64).reshape(-1)
    if p.size != 16:
        raise ValueError("two_view_pose: pose must hold 16 numbers, got %d" % p.size)
    R, t = p[:9].reshape(3, 3).copy(), p[9:12].copy()
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    sin2 = float(np.sqrt(v @ v))
    cand = int(p[15])
    angle = float(np.degrees(np.arctan2(0.5 * sin2, 0.5 * (np.trace(R) - 1.0)))) if cand >= 0 else 0.0
    return dict(R=R, t=t, angle_deg=angle, axis=v / sin2 if cand >= 0 and sin2 > 0.0 else None, singular=p[12:15].copy(), candidate=cand)


# ---------------------------------------------------------------------- superpixels and per-segment models (csrc/superpixels.hip)
SUPERPIXEL_COUNTS = ("centres", "empty_centres", "components", "small", "pixels_merged", "n_seg", "largest", "reserved")
SEGMENT_FIT_COUNTS = ("part", "agree", "with_model", "affine", "translation", "bad_label", "out_of_range", "reserved")


def _int_in(fn, name, v, lo, hi):
    if not (isinstance(v, (int, np.integer)) and not isinstance(v, bool) and lo <= v <= hi):
        raise ValueError("%s: %s must be an int in [%d, %d], got %r" % (fn, name, lo, hi, v))
    return int(v)


def _superpixels_gate(fn, img, step, compactness, iters, min_size):
    """The arguments of superpixels through the input gate, before any device is touched: (img, min_size)."""
    img = _check(img, fn, "img", torch.uint8, (None, None, 3))
    H, W, _ = img.shape
    if not (1 <= H <= 8192 and 1 <= W <= 8192):
        raise ValueError("%s: img must be between 1x1 and 8192x8192, got %dx%d" % (fn, W, H))
    step = _int_in(fn, "step", step, 4, 64)
    _int_in(fn, "compactness", compactness, 0, 255)
    _int_in(fn, "iters", iters, 1, 32)
    return img, step * step // 4 if min_size is None else _int_in(fn, "min_size", min_size, 0, _lib.SEGMENTS_MAX)


def _segment_fit_gate(fn, flow, thresh, rounds, shape=None):
    """flow, thresh and rounds of segment_fit through the input gate: the flow, of frame size `shape` if that is given."""
    flow = _check(flow, fn, "flow", torch.float32, (None, None, (2, 3)) if shape is None else (shape[0], shape[1], (2, 3)))
    if not (1 <= flow.shape[0] <= 8192 and 1 <= flow.shape[1] <= 8192):
        raise ValueError("%s: flow must be between 1x1 and 8192x8192, got %dx%d" % (fn, flow.shape[1], flow.shape[0]))
    if not (isinstance(thresh, (int, float, np.integer, np.floating)) and np.isfinite(np.float32(thresh)) and np.float32(thresh) > 0):
        raise ValueError("%s: thresh must be finite and > 0 as a float32, got %r" % (fn, thresh))
    _int_in(fn, "rounds", rounds, 1, 6)
    return flow


def superpixel_grid(h, w, step):
    """(gh, gw, K) of dflow_superpixels: the rows, the columns and the number of the grid's centres."""
    gh, gw = -(-int(h) // int(step)), -(-int(w) // int(step))
    return gh, gw, gh * gw


def _superpixels_call(img, step, compactness, iters, min_size, slic, counts):
    """One dflow_superpixels on a device image into new planes: (labels, centers, slic or None, counts or None)."""
    H, W, _ = img.shape
    dev = img.device
    K = superpixel_grid(H, W, step)[2]
    i32 = torch.int32
    label, centers = torch.empty((H, W), dtype=i32, device=dev), torch.empty((K, 8), dtype=i32, device=dev)
    raw, cnt = _out(slic, (H, W), i32, dev), _out(counts, 8, i32, dev)
    sums, scan = torch.empty((K, 8), dtype=i32, device=dev), torch.empty(-(-(H * W) // 256) + 1, dtype=i32, device=dev)
    comp, size, fin = (torch.empty((H, W), dtype=i32, device=dev) for _ in range(3))
    _lib.call("dflow_superpixels", H, W, img.data_ptr(), int(step), int(compactness), int(iters), int(min_size), 0, label.data_ptr(),
              centers.data_ptr(), _ptr(raw), _ptr(cnt), sums.data_ptr(), comp.data_ptr(), size.data_ptr(), fin.data_ptr(),
              scan.data_ptr(), _lib.stream(dev))
    return label, centers, raw, cnt


def superpixels(img, step=16, compactness=10, iters=10, min_size=None, centers=False, slic=False, counts=False):
    """An over-segmentation of an image into compact regions of similar colour (dflow_superpixels, DESIGN.md "Superpixels and
    per-segment flow models"): an integer gSLIC on a grid of `step` pixels, `iters` iterations, spatial weight `compactness`
    (0: colour alone), whose segments are 4-connected, have at least min_size pixels (None: step*step//4; but for the segment
    that holds pixel 0) and are numbered 0 .. n_seg-1 in raster order of their first pixels.  img is an (H,W,3) uint8 BGR device
    tensor or host array; host data is uploaded to the current device.  Returns the (H,W) int32 device plane of segment numbers,
    or a tuple in the order (labels[, centers][, slic][, counts]): centers=True adds the (K,8) int32 centres [cx16, cy16, b16,
    g16, r16, n, 0, 0], slic=True the raw (H,W) int32 SLIC labels, counts=True the int32[8] device tensor SUPERPIXEL_COUNTS, whose
    entry 5 is n_seg.  Runs on torch's current stream and does not wait for it."""
    img, min_size = _superpixels_gate("superpixels", img, step, compactness, iters, min_size)
    dev = _device_of(img)
    img, = _on(dev, img)
    label, cen, raw, cnt = _superpixels_call(img, step, compactness, iters, min_size, slic, counts)
    ret = (label,) + tuple(t for t, want in ((cen, centers), (raw, slic), (cnt, counts)) if want)
    return ret if len(ret) > 1 else label


def _segment_fit_call(flow, labels, n_seg, thresh, rounds, out, classes, counts):
    """One dflow_segment_fit on device tensors into new planes: (models, seg_counts, [out, classes, counts] or Nones)."""
    H, W, _ = flow.shape
    dev = flow.device
    models = torch.empty((n_seg, 6), dtype=torch.float32, device=dev)
    seg_counts = torch.empty((n_seg, 4), dtype=torch.int32, device=dev)
    acc = torch.empty((n_seg, 12), dtype=torch.int64, device=dev)
    extra = [_out(out, (H, W, 3), torch.float32, dev), _out(classes, (H, W), torch.uint8, dev), _out(counts, 8, torch.int32, dev)]
    _lib.call("dflow_segment_fit", H, W, flow.data_ptr(), _layout(flow), labels.data_ptr(), int(n_seg), float(thresh), int(rounds), 0,
              models.data_ptr(), seg_counts.data_ptr(), _ptr(extra[0]), _ptr(extra[1]), _ptr(extra[2]), acc.data_ptr(), _lib.stream(dev))
    return models, seg_counts, extra


def segment_fit(flow, labels, n_seg, thresh=1.0, rounds=3, out=False, classes=False, counts=False):
    """A robust affine flow model per segment (dflow_segment_fit, DESIGN.md "Superpixels and per-segment flow models"): least
    squares over the vectors of each segment, trimmed in `rounds` rounds whose thresholds halve down to thresh pixels; a segment
    with fewer than three vectors or with vectors on one line gets their mean, one with none no model.  flow is (H,W,2) float32
    [dy,dx] or (H,W,3) float32 [U,V,valid]; labels an (H,W) int32 plane, any labelling (superpixels', a mask, a motion layer
    plane cast to int32), of which the values in [0, n_seg) are segments.  Device tensors or host arrays; host data is uploaded
    to the current device.  Returns (models, seg_counts), the (n_seg,6) float32 models [m0..m5], U = m0 x + m1 y + m2, V = m3 x +
    m4 y + m5, and the (n_seg,4) int32 {pixels, vectors that take part, those that agree, kind: 0 none / 1 translation / 2
    affine}, followed in this order by what is asked for: out=True the (H,W,3) float32 [U,V,valid] flow of the models (holes
    inside a segment are filled), classes=True the (H,W) uint8 plane 0 takes no part / 1 agrees / 2 disagrees / 3 no model,
    counts=True the int32[8] device tensor SEGMENT_FIT_COUNTS.  Runs on torch's current stream and does not wait for it."""
    fn = "segment_fit"
    flow = _segment_fit_gate(fn, flow, thresh, rounds)
    labels = _check(labels, fn, "labels", torch.int32, (flow.shape[0], flow.shape[1]))
    n_seg = _int_in(fn, "n_seg", n_seg, 1, _lib.SEGMENTS_MAX)
    dev = _device_of(flow, labels)
    flow, labels = _on(dev, flow, labels)
    models, seg_counts, extra = _segment_fit_call(flow, labels, n_seg, thresh, rounds, out, classes, counts)
    return (models, seg_counts) + tuple(t for t in extra if t is not None)


def superpixel_flow(img, flow, step=16, compactness=10, iters=10, min_size=None, thresh=1.0, rounds=3, classes=False, counts=False):
    """superpixels on img, then segment_fit of flow on its segments: the piecewise-affine version of a flow field.  The
    per-segment planes are sized from the n_seg this function reads back once (it waits for the stream there); the library reads
    nothing back.  Returns (labels, models, seg_counts, out[, classes][, counts]) as the two functions define them; n_seg is
    models.shape[0]."""
    fn = "superpixel_flow"
    img, min_size = _superpixels_gate(fn, img, step, compactness, iters, min_size)
    flow = _segment_fit_gate(fn, flow, thresh, rounds, shape=img.shape)
    dev = _device_of(img, flow)
    img, flow = _on(dev, img, flow)
    label, _, _, cnt = _superpixels_call(img, step, compactness, iters, min_size, False, True)
    n_seg = int(cnt[5].item())
    models, seg_counts, extra = _segment_fit_call(flow, label, n_seg, thresh, rounds, True, classes, counts)
    return (label, models, seg_counts) + tuple(t for t in extra if t is not None)


# ---------------------------------------------------------------------- point trajectories (csrc/tracks.hip)
TRACK_STATES = ("free", "live", "left", "noflow", "noback", "inconsistent")
TRACK_ADVANCE_COUNTS = ("live", "left", "noflow", "noback", "inconsistent", "not_live")
TRACK_SEED_COUNTS = ("covered", "seedable", "seeded", "dropped")
TRACK_FLOW_COUNTS = ("set", "lost", "no_part")


def track_scan_len(h, w, step):
    """The int32 elements of dflow_track_seed's d_scan for an (h, w) frame: the cells, a sum per 1024 cells, one more."""
    ncells = -(-int(h) // int(step)) * -(-int(w) // int(step))
    return ncells + -(-ncells // 1024) + 1


def _track_frame(fn, h, w):
    for name, v in (("h", h), ("w", w)):
        if not (isinstance(v, (int, np.integer)) and 1 <= v <= 8192):
            raise ValueError("%s: %s must be an int in [1, 8192], got %r" % (fn, name, v))
    return int(h), int(w)


def _track_set(fn, pos, state, names=("pos", "state"), cap=None):
    """A set's positions and states through the input gate: (cap,2) float32 and (cap) int32, 1 <= cap <= 2^26."""
    pos = _check(pos, fn, names[0], torch.float32, (cap, 2))
    cap = pos.shape[0]
    if not 1 <= cap <= _lib.TRACK_CAP_MAX:
        raise ValueError("%s: a track set holds 1 to 2^26 slots, got %d" % (fn, cap))
    return pos, _check(state, fn, names[1], torch.int32, (cap,))


def _track_tol(fn, name, v):
    if not isinstance(v, (int, float, np.integer, np.floating)) or not (np.isfinite(np.float32(v)) and np.float32(v) >= 0):
        raise ValueError("%s: %s must be finite and >= 0 as a float32, got %r" % (fn, name, v))
    return float(np.float32(v))


def _track_planes(dev, *tensors):
    """The tensors on `dev`, contiguous, on an 8-byte boundary (a row of a stack of snapshots is, its positions being float2);
    a caller's device tensor that is all that stays the caller's, so that dflow_track_seed writes into it."""
    out = [t.to(dev).contiguous() for t in tensors]
    return [t.clone() if t.data_ptr() % 8 else t for t in out]


def track_advance(h, w, pos, state, fwd, bwd=None, rel=0.01, abs=0.5, inplace=False, err=False, counts=False):
    """A track set carried one frame forward (dflow_track_advance, DESIGN.md "Point trajectories"): every LIVE track moves by
    the bilinear sample of the forward flow at its position, and ends, keeping its position, when it leaves the (h, w) frame
    (LEFT), meets a forward vector that is not good (NOFLOW), or, with bwd, meets a backward vector that is not good (NOBACK) or
    fails e2 <= rel * m2 + abs, e2 = |f + b|^2, m2 = |f|^2 + |b|^2 (INCONSISTENT).  pos is (cap,2) float32 [x,y], state (cap)
    int32 (TRACK_STATES); fwd and bwd are (h,w,2) float32 [dy,dx] or (h,w,3) float32 [U,V,valid], each on its own.  Device
    tensors or host arrays; host data is uploaded to the current device.  Returns (pos, state[, err][, counts]): new device
    tensors, or with inplace=True the set's own where those are device tensors; err=True adds the (cap) float32 plane of e2 (-1
    where it was not formed), counts=True the int32[6] device tensor TRACK_ADVANCE_COUNTS.  Runs on torch's current stream and
    does not wait for it."""
    fn = "track_advance"
    h, w = _track_frame(fn, h, w)
    pos, state = _track_set(fn, pos, state)
    fwd = _check(fwd, fn, "fwd", torch.float32, (h, w, (2, 3)))
    if bwd is not None:
        bwd = _check(bwd, fn, "bwd", torch.float32, (h, w, (2, 3)))
    rel, abs = _track_tol(fn, "rel", rel), _track_tol(fn, "abs", abs)
    dev = _device_of(pos, state, fwd, *([bwd] if bwd is not None else []))
    ts = _on(dev, fwd, *([bwd] if bwd is not None else []))
    fwd, bwd = ts[0], ts[1] if bwd is not None else None
    pos, state = _track_planes(dev, pos, state)
    cap = pos.shape[0]
    pos_out, state_out = (pos, state) if inplace else (torch.empty_like(pos), torch.empty_like(state))
    extra = [_out(err, cap, torch.float32, dev), _out(counts, 6, torch.int32, dev)]
    _lib.call("dflow_track_advance", h, w, fwd.data_ptr(), _layout(fwd), _ptr(bwd), _layout(bwd) if bwd is not None else 0, cap,
              pos.data_ptr(), state.data_ptr(), rel, abs, 0, pos_out.data_ptr(), state_out.data_ptr(), _ptr(extra[0]), _ptr(extra[1]),
              _lib.stream(dev))
    return tuple(t for t in [pos_out, state_out] + extra if t is not None)


def track_seed(h, w, pos, state, birth, n, step=4, frame=0, mask=None, counts=False, scan=None):
    """New tracks where no live one is (dflow_track_seed): the frame is cut into step x step cells; every cell that holds no
    LIVE track among the first n slots, and whose centre pixel is non-zero in mask ((h,w) uint8, or None), starts a track at its
    centre pixel in the next free slot, in raster order, with birth = frame; cells beyond the set's capacity are dropped.  pos
    (cap,2) float32, state (cap) int32, birth (cap) int32; n the int32[1] tensor of the slots handed out so far, or an int.
    Device tensors or host arrays; the set is written in place where it is given as contiguous device tensors, and is returned
    either way: (pos, state, birth, n[, counts]), n an int32[1] device tensor, counts=True adding the int32[4] device tensor
    TRACK_SEED_COUNTS.  scan: an int32 device tensor of track_scan_len(h, w, step) elements to reuse, or None.  Runs on
    torch's current stream and does not wait for it."""
    fn = "track_seed"
    h, w = _track_frame(fn, h, w)
    pos, state = _track_set(fn, pos, state)
    cap = pos.shape[0]
    birth = _check(birth, fn, "birth", torch.int32, (cap,))
    if not (isinstance(step, (int, np.integer)) and 1 <= step <= 256):
        raise ValueError("%s: step must be an int in [1, 256], got %r" % (fn, step))
    if not (isinstance(frame, (int, np.integer)) and -2 ** 31 <= frame < 2 ** 31):
        raise ValueError("%s: frame must be an int32, got %r" % (fn, frame))
    if isinstance(n, (int, np.integer)):
        n = torch.tensor([min(max(int(n), -2 ** 31), 2 ** 31 - 1)], dtype=torch.int32)
    n = _check(n, fn, "n", torch.int32, (1,))
    if mask is not None:
        mask = _check(mask, fn, "mask", torch.uint8, (h, w))
    need = track_scan_len(h, w, step)
    if scan is not None and not (isinstance(scan, torch.Tensor) and scan.dtype == torch.int32 and scan.dim() == 1 and scan.numel() >= need
                                 and scan.is_contiguous() and scan.is_cuda):
        raise ValueError("%s: scan must be a contiguous int32 device tensor of at least %d elements" % (fn, need))
    dev = _device_of(pos, state, birth, n, *([scan] if scan is not None else []))
    pos, state, birth, n = _track_planes(dev, pos, state, birth, n)
    if mask is not None:
        mask, = _on(dev, mask)
    if scan is None:
        scan = torch.empty(need, dtype=torch.int32, device=dev)
    cnt = _out(counts, 4, torch.int32, dev)
    _lib.call("dflow_track_seed", h, w, cap, int(step), int(frame), _ptr(mask), pos.data_ptr(), state.data_ptr(), birth.data_ptr(),
              n.data_ptr(), scan.data_ptr(), _ptr(cnt), _lib.stream(dev))
    return (pos, state, birth, n) + ((cnt,) if counts else ())


def track_flow(h, w, pos_a, state_a, pos_b, state_b, owner=False, counts=False):
    """The sparse flow a -> b of the tracks that are LIVE in two snapshots of one set (dflow_track_flow): every such track whose
    position in a lies inside the frame claims the pixel nearest to it, the smallest index winning a shared pixel, and the pixel
    receives [x_b - x_a, y_b - y_a, 1]; every other pixel is [0,0,0].  The (h,w,3) float32 [U,V,valid] field is what
    epic_interpolate, segment_filter and flow_eval take.  Snapshots: (cap,2) float32 and (cap) int32, device tensors or host
    arrays.  Returns the device tensor, or a tuple in the order (flow[, owner][, counts]): owner=True adds the (h,w) int32 plane
    of winners (0x7fffffff: none), counts=True the int32[3] device tensor TRACK_FLOW_COUNTS.  Runs on torch's current stream
    and does not wait for it."""
    fn = "track_flow"
    h, w = _track_frame(fn, h, w)
    pos_a, state_a = _track_set(fn, pos_a, state_a, ("pos_a", "state_a"))
    pos_b, state_b = _track_set(fn, pos_b, state_b, ("pos_b", "state_b"), cap=pos_a.shape[0])
    dev = _device_of(pos_a, state_a, pos_b, state_b)
    pos_a, state_a, pos_b, state_b = _track_planes(dev, pos_a, state_a, pos_b, state_b)
    own = torch.empty((h, w), dtype=torch.int32, device=dev)
    out = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
    cnt = _out(counts, 3, torch.int32, dev)
    _lib.call("dflow_track_flow", h, w, pos_a.shape[0], pos_a.data_ptr(), state_a.data_ptr(), pos_b.data_ptr(), state_b.data_ptr(),
              own.data_ptr(), out.data_ptr(), _ptr(cnt), _lib.stream(dev))
    ret = tuple(t for t in (out, own if owner else None, cnt) if t is not None)
    return ret if len(ret) > 1 else out


class TrackSet:
    """Point trajectories through a frame sequence, on the device: seed() starts tracks at the current frame, advance(fwd, bwd)
    carries the set to the next frame and keeps a snapshot per frame, flow(a, b) is the sparse flow between two frames' snapshots,
    read() the one read-back.  Slots are never reused, so index i is one trajectory in every snapshot.  cap defaults to four
    times the number of step x step cells."""

    def __init__(self, h, w, cap=None, step=4, rel=0.01, abs=0.5, device=None):
        fn = "TrackSet"
        self.h, self.w = _track_frame(fn, h, w)
        if not (isinstance(step, (int, np.integer)) and 1 <= step <= 256):
            raise ValueError("%s: step must be an int in [1, 256], got %r" % (fn, step))
        self.step = int(step)
        if cap is None:
            cap = min(4 * -(-self.h // self.step) * -(-self.w // self.step), _lib.TRACK_CAP_MAX)
        if not (isinstance(cap, (int, np.integer)) and 1 <= cap <= _lib.TRACK_CAP_MAX):
            raise ValueError("%s: cap must be an int in [1, 2^26], got %r" % (fn, cap))
        self.cap = int(cap)
        self.rel, self.abs = _track_tol(fn, "rel", rel), _track_tol(fn, "abs", abs)
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self.pos = torch.zeros((self.cap, 2), dtype=torch.float32, device=dev)
        self.state = torch.zeros(self.cap, dtype=torch.int32, device=dev)
        self.birth = torch.zeros(self.cap, dtype=torch.int32, device=dev)
        self.n = torch.zeros(1, dtype=torch.int32, device=dev)
        self.scan = torch.empty(track_scan_len(self.h, self.w, self.step), dtype=torch.int32, device=dev)
        self.frame = 0
        self.snapshots = [(self.pos, self.state)]     # per frame; the last one is the current set, which seed() writes
        self._counts = {"seed": None, "advance": None}

    def seed(self, mask=None):
        """Starts a track in every cell no live track covers (track_seed) at the current frame."""
        out = track_seed(self.h, self.w, self.pos, self.state, self.birth, self.n, step=self.step, frame=self.frame, mask=mask,
                         counts=True, scan=self.scan)
        assert out[0].data_ptr() == self.pos.data_ptr() and out[3].data_ptr() == self.n.data_ptr()
        self._counts["seed"] = out[4]
        return self

    def advance(self, fwd, bwd=None):
        """Carries the set along fwd (the flow from the current frame to the next; bwd the flow back, or None for no check) and
        makes the result the current frame."""
        pos, state, cnt = track_advance(self.h, self.w, self.pos, self.state, fwd, bwd, rel=self.rel, abs=self.abs, counts=True)
        self.pos, self.state = pos, state
        self.snapshots.append((pos, state))
        self.frame += 1
        self._counts["advance"] = cnt
        return self

    def seed_corners(self, pyr, **corner_args):
        """Starts a track at every corner of the pyramid's level 0 (corners) that no live track of the set suppresses, at the
        current frame.  The set must have been built with step=1: a corner is a pixel, and a cell must be one."""
        if self.step != 1:
            raise ValueError("TrackSet.seed_corners: the set must be built with step=1 (a corner is one pixel), this one has step=%d" % self.step)
        for name in ("tracks", "response", "counts"):
            if name in corner_args:
                raise ValueError("TrackSet.seed_corners: %s is not an argument here" % name)
        mask, cnt = corners(pyr, self.h, self.w, tracks=(self.pos, self.state, self.n), counts=True, **corner_args)
        self._counts["corners"] = cnt
        return self.seed(mask)

    def advance_klt(self, pyr1, pyr2, levels=None, **klt_args):
        """Carries the set from the frame of pyr1 to the frame of pyr2 by pyramidal Lucas-Kanade (klt_track) and makes the result
        the current frame: snapshots, frame counter and counts as in advance().  levels: those of the two klt_pyramid buffers;
        None reads it off the length of pyr1."""
        for name in ("inplace", "err", "counts"):
            if name in klt_args:
                raise ValueError("TrackSet.advance_klt: %s is not an argument here" % name)
        if levels is None:
            fit = [k for k in range(1, _lib.KLT_LEVELS_MAX + 1) if klt_pyramid_len(self.h, self.w, k) == len(pyr1)]
            if not fit:
                raise ValueError("TrackSet.advance_klt: pyr1 holds %d bytes, no pyramid of a %dx%d frame does" % (len(pyr1), self.w, self.h))
            levels = fit[0]
        pos, state, cnt = klt_track(pyr1, pyr2, self.h, self.w, levels, self.pos, self.state, counts=True, **klt_args)
        self.pos, self.state = pos, state
        self.snapshots.append((pos, state))
        self.frame += 1
        self._counts["advance"] = cnt
        return self

    def flow(self, a, b, owner=False, counts=False):
        """The sparse flow from frame a to frame b (track_flow) of the tracks alive in both."""
        for name, v in (("a", a), ("b", b)):
            if not (isinstance(v, (int, np.integer)) and 0 <= v <= self.frame):
                raise ValueError("TrackSet.flow: %s must be a frame in [0, %d], got %r" % (name, self.frame, v))
        (pa, sa), (pb, sb) = self.snapshots[a], self.snapshots[b]
        return track_flow(self.h, self.w, pa, sa, pb, sb, owner=owner, counts=counts)

    def counts(self):
        """The int32 device tensors of the last seed() (TRACK_SEED_COUNTS) and the last advance() (TRACK_ADVANCE_COUNTS), None
        where there was none: {"seed": ..., "advance": ...}.  After seed_corners() there is "corners" (CORNER_COUNTS) as well, and
        after advance_klt() "advance" holds KLT_TRACK_COUNTS.  Nothing is read back."""
        return dict(self._counts)

    def read(self):
        """The one read-back: dict(pos (T,n,2) float32, NaN before a track's birth and its last position repeated after its
        end; state (T,n) int32; birth (n) int32; length (n) int32, the frames a track is live in), T = frames so far, n = slots
        handed out."""
        n = min(max(int(self.n.cpu()[0]), 0), self.cap)
        pos = torch.stack([p[:n] for p, _ in self.snapshots]).cpu().numpy()
        state = torch.stack([s[:n] for _, s in self.snapshots]).cpu().numpy()
        birth = self.birth[:n].cpu().numpy()
        pos[np.arange(len(self.snapshots))[:, None] < birth[None, :]] = np.nan
        return dict(pos=pos, state=state, birth=birth, length=(state == _lib.TRACK_LIVE).sum(0).astype(np.int32))


# ---------------------------------------------------------------------- sparse feature tracking (csrc/klt.hip)
TRACK_STATES_KLT = TRACK_STATES + ("flat", "residual")
CORNER_COUNTS = ("candidates", "maxima", "suppressed", "corners")
KLT_TRACK_COUNTS = ("live", "left", "flat", "residual", "inconsistent", "not_live", "converged", "reserved")


def klt_pyramid_len(h, w, levels):
    """The bytes of the grey pyramid of an (h, w) frame: level l is ((h_l+1)//2, (w_l+1)//2) of level l-1, one after the other."""
    total = 0
    for _ in range(int(levels)):
        total += int(h) * int(w)
        h, w = (int(h) + 1) // 2, (int(w) + 1) // 2
    return total


def _klt_levels(fn, levels):
    if not (isinstance(levels, (int, np.integer)) and 1 <= levels <= _lib.KLT_LEVELS_MAX):
        raise ValueError("%s: levels must be an int in [1, %d], got %r" % (fn, _lib.KLT_LEVELS_MAX, levels))
    return int(levels)


def _klt_float(fn, name, v, positive=False):
    ok = isinstance(v, (int, float, np.integer, np.floating)) and np.isfinite(np.float32(v))
    if not ok or not (np.float32(v) > 0 if positive else np.float32(v) >= 0):
        raise ValueError("%s: %s must be finite and %s 0 as a float32, got %r" % (fn, name, ">" if positive else ">=", v))
    return float(np.float32(v))


def klt_pyramid(img, levels=3):
    """The grey pyramid of a (H,W,3) uint8 BGR image (dflow_klt_pyramid, DESIGN.md "Sparse feature tracking"): level 0 is
    (29 b + 150 g + 77 r + 128) >> 8, every further level pyr_down's 5x5 binomial of the one before at half the size.  Returns one
    uint8 device tensor of klt_pyramid_len(H, W, levels) bytes, the levels one after the other: what corners and klt_track take.
    A device tensor or a host array; runs on torch's current stream and does not wait for it."""
    fn = "klt_pyramid"
    img = _check(img, fn, "img", torch.uint8, (None, None, 3))
    levels = _klt_levels(fn, levels)
    H, W = _track_frame(fn, img.shape[0], img.shape[1])
    dev = _device_of(img)
    img, = _on(dev, img)
    pyr = torch.empty(klt_pyramid_len(H, W, levels), dtype=torch.uint8, device=dev)
    _lib.call("dflow_klt_pyramid", H, W, levels, img.data_ptr(), pyr.data_ptr(), _lib.stream(dev))
    return pyr


def _klt_pyr(fn, name, pyr, h, w, levels):
    pyr = _check(pyr, fn, name, torch.uint8, (None,))
    if pyr.numel() < klt_pyramid_len(h, w, levels):
        raise ValueError("%s: %s holds %d bytes, a %dx%d pyramid of %d levels has %d" % (fn, name, pyr.numel(), w, h, levels,
                                                                                          klt_pyramid_len(h, w, levels)))
    return pyr


def corners(pyr, h, w, rc=2, min_dist=4, border=4, quality=0.01, min_response=0.0, tracks=None, response=False, counts=False):
    """Shi-Tomasi corners of level 0 of a pyramid (dflow_corners): R is the smaller eigenvalue of the structure tensor of the
    central differences over the (2 rc + 1)^2 window; a corner is a pixel at least `border` from the frame's edge with R > 0,
    R >= quality * max R and R >= min_response that is the maximum of its (2 min_dist + 1)^2 neighbourhood (ties: the smaller
    raster index) and has no live track of `tracks` = (pos, state, n), a track set as track_seed takes it, in that
    neighbourhood.  Returns the (h,w) uint8 mask, 255 at a corner: what track_seed(step=1, mask=...) turns into tracks, in raster
    order; or a tuple (mask[, response][, counts]): the (h,w) float32 plane of R, the int32[4] device tensor CORNER_COUNTS.
    Runs on torch's current stream and does not wait for it."""
    fn = "corners"
    h, w = _track_frame(fn, h, w)
    pyr = _klt_pyr(fn, "pyr", pyr, h, w, 1)
    rc, min_dist, border = _int_in(fn, "rc", rc, 1, 7), _int_in(fn, "min_dist", min_dist, 1, 32), _int_in(fn, "border", border, 0, 8192)
    quality, min_response = _klt_float(fn, "quality", quality), _klt_float(fn, "min_response", min_response)
    if quality > 1:
        raise ValueError("%s: quality must be in [0, 1], got %r" % (fn, quality))
    pos = state = n = None
    if tracks is not None:
        pos, state = _track_set(fn, tracks[0], tracks[1])
        n = tracks[2]
        if isinstance(n, (int, np.integer)):
            n = torch.tensor([min(max(int(n), -2 ** 31), 2 ** 31 - 1)], dtype=torch.int32)
        n = _check(n, fn, "n", torch.int32, (1,))
    dev = _device_of(pyr, *([pos, state, n] if tracks is not None else []))
    pyr, = _on(dev, pyr)
    occ = None
    if tracks is not None:
        pos, state, n = _track_planes(dev, pos, state, n)
        occ = torch.empty((h, w), dtype=torch.uint8, device=dev)
    resp = torch.empty((h, w), dtype=torch.float32, device=dev)
    mask = torch.empty((h, w), dtype=torch.uint8, device=dev)
    rmax = torch.empty(1, dtype=torch.int32, device=dev)
    cnt = _out(counts, 4, torch.int32, dev)
    _lib.call("dflow_corners", h, w, pyr.data_ptr(), rc, min_dist, border, quality, min_response, pos.shape[0] if tracks is not None else 0,
              _ptr(pos), _ptr(state), _ptr(n), resp.data_ptr(), mask.data_ptr(), _ptr(occ), rmax.data_ptr(), _ptr(cnt), _lib.stream(dev))
    ret = tuple(t for t in (mask, resp if response else None, cnt) if t is not None)
    return ret if len(ret) > 1 else mask


def klt_track(pyr1, pyr2, h, w, levels, pos, state, r=7, iters=20, eps=0.01, min_eig=1.0, max_err=0.0, fb=0.5, inplace=False,
              err=False, counts=False):
    """A track set carried from the frame of pyr1 to the frame of pyr2 by pyramidal Lucas-Kanade (dflow_klt_track): every LIVE
    track is followed through the `levels` levels of the two klt_pyramid buffers with a (2r+1)^2 window, at most `iters`
    Gauss-Newton steps per level, stopping below `eps` pixels.  It ends, keeping its position, when it leaves the frame (LEFT), when
    the smaller eigenvalue of its window's gradient matrix is below min_eig grey^2/px^2 at level 0 (FLAT), when its mean absolute
    residual exceeds max_err grey levels (RESIDUAL; 0: no test), or when tracking back from pyr2 to pyr1 does not return within fb
    pixels (INCONSISTENT; 0: no backward pass).  pos (cap,2) float32 [x,y], state (cap) int32 (TRACK_STATES_KLT); device tensors
    or host arrays.  Returns (pos, state[, err][, counts]) as track_advance does: err=True adds the (cap) float32 residual (-1
    where none was formed), counts=True the int32[8] device tensor KLT_TRACK_COUNTS.  Runs on torch's current stream and does not
    wait for it."""
    fn = "klt_track"
    h, w = _track_frame(fn, h, w)
    levels = _klt_levels(fn, levels)
    pyr1, pyr2 = _klt_pyr(fn, "pyr1", pyr1, h, w, levels), _klt_pyr(fn, "pyr2", pyr2, h, w, levels)
    pos, state = _track_set(fn, pos, state)
    r, iters = _int_in(fn, "r", r, 1, 10), _int_in(fn, "iters", iters, 1, 64)
    eps = _klt_float(fn, "eps", eps, positive=True)
    min_eig, max_err, fb = _klt_float(fn, "min_eig", min_eig), _klt_float(fn, "max_err", max_err), _klt_float(fn, "fb", fb)
    dev = _device_of(pos, state, pyr1, pyr2)
    pyr1, pyr2 = _on(dev, pyr1, pyr2)
    pos, state = _track_planes(dev, pos, state)
    cap = pos.shape[0]
    pos_out, state_out = (pos, state) if inplace else (torch.empty_like(pos), torch.empty_like(state))
    extra = [_out(err, cap, torch.float32, dev), _out(counts, 8, torch.int32, dev)]
    _lib.call("dflow_klt_track", h, w, levels, pyr1.data_ptr(), pyr2.data_ptr(), cap, pos.data_ptr(), state.data_ptr(), r, iters, eps,
              min_eig, max_err, fb, 0, pos_out.data_ptr(), state_out.data_ptr(), _ptr(extra[0]), None, _ptr(extra[1]), _lib.stream(dev))
    return tuple(t for t in [pos_out, state_out] + extra if t is not None)


def klt_sparse_flow(img1, img2, levels=3, cap=None, corner_args=None, **klt_args):
    """The sparse flow img1 -> img2 without a dense pass: pyramids -> corners -> klt_track -> track_flow.  Returns the (H,W,3)
    float32 [U,V,valid] device tensor epic_interpolate, motion_fit, epipolar_fit, segment_filter and flow_eval take, valid at the
    corners of img1 whose track is live in img2.  cap: the most corners that are followed (default: one per 16 pixels)."""
    fn = "klt_sparse_flow"
    img1 = _check(img1, fn, "img1", torch.uint8, (None, None, 3))
    H, W = img1.shape[0], img1.shape[1]
    img2 = _check(img2, fn, "img2", torch.uint8, (H, W, 3))
    ts = TrackSet(H, W, cap=cap if cap is not None else max(1, H * W // 16), step=1, device=_device_of(img1, img2))
    pyr1, pyr2 = klt_pyramid(img1, levels), klt_pyramid(img2, levels)
    ts.seed_corners(pyr1, **(corner_args or {}))
    ts.advance_klt(pyr1, pyr2, levels=levels, **klt_args)
    return ts.flow(0, 1)


def pyramid_levels(pich, picw, levels=2, cellh=None, cellw=None, fine_window=None, **overrides):
    """The geometry of a coarse-to-fine run, level 0 the finest: a list of dicts of DiscreteFlow's arguments (pich, picw, cellh,
    cellw and the overrides).  THE RULE: level l+1 has the size ((H+1)//2, (W+1)//2) of level l and the SAME cell size in pixels
    as level 0, clipped to its image, so a cell covers twice the scene per level and the reach of the +-window-cell search
    doubles with it.  All coarse levels keep `window` as given (the library's default without it); level 0 takes fine_window
    when that is not None.  ValueError, naming the level, for a level the library would refuse (an image below 8 px, a cell
    with fewer than knn points, a window outside [0,2], ...).  Needs the library, not a device."""
    levels = int(levels)
    if levels < 1:
        raise ValueError("PyramidFlow: levels must be >= 1, got %d" % levels)
    if cellh is None or cellw is None:
        cellh, cellw = default_cells(pich, picw)
    out, H, W = [], int(pich), int(picw)
    for level in range(levels):
        over = dict(overrides)
        if level == 0 and fine_window is not None:
            over["window"] = int(fine_window)
        geom = dict(pich=H, picw=W, cellh=min(int(cellh), H), cellw=min(int(cellw), W))
        p = _lib.default_params(geom["pich"], geom["picw"], geom["cellh"], geom["cellw"], **over)
        if not _lib.lib().dflow_workspace_bytes(C.byref(p)):
            raise ValueError("PyramidFlow: level %d (%dx%d, cells %dx%d) is refused: %s"
                             % (level, W, H, geom["cellw"], geom["cellh"], _lib.lib().dflow_last_error().decode()))
        out.append(dict(geom, **over))
        H, W = (H + 1) // 2, (W + 1) // 2
    return out


def image_pyramid(levels, pic3, pic4):
    """[(img1, img2)] per DiscreteFlow of `levels` (level 0, the finest, first) as device tensors: one dflow_pyr_down launch per
    coarse level, for both images."""
    df = levels[0]
    pyr = [(df._device_image(pic3, df._img), df._device_image(pic4, df._img2))]
    for _ in levels[1:]:
        pyr.append(pyr_down(*pyr[-1]))
    return pyr


class PyramidFlow:
    """Coarse-to-fine passes (DESIGN.md "Coarse to fine"): one DiscreteFlow per level (self.levels, level 0 the finest, geometry
    by pyramid_levels' rule); the coarsest level runs as DiscreteFlow.run does, every finer one starts from the upsampled flow of
    the next coarser level, level l from level l + 1 (flow_upsample -> prior_proposals).  A vector beyond level 0's search window can enter its label sets
    this way, and with a believed prior level 0 may search fewer cells (fine_window 1 or 0)."""

    def __init__(self, pich, picw, levels=2, cellh=None, cellw=None, device="cuda:0", seed=0, fine_window=None, **overrides):
        geoms = pyramid_levels(pich, picw, levels, cellh, cellw, fine_window, **overrides)
        self.levels = [DiscreteFlow(device=device, seed=seed, **g) for g in geoms]
        self.device = self.levels[0].device
        self.counts = []
        self.gate_counts = []

    def size(self, level):
        p = self.levels[level].p
        return p.pich, p.picw

    def image_pyramid(self, pic3, pic4):
        """The module's image_pyramid for this run's levels."""
        return image_pyramid(self.levels, pic3, pic4)

    def run_level(self, level, imgs, bcd_times, prior=None, prior_stride=2, seed_labels=True, counts=False):
        """One level's pass on its images; prior None: the calls of DiscreteFlow.run.  Returns (the level's flow tensor, the int32[4] counts of
        its prior step as a device tensor, or None without a prior or with counts=False)."""
        df = self.levels[level]
        cnt = df.front_end(imgs[0], imgs[1], prior, prior_stride, seed_labels, counts)
        df.ceoBCD(bcd_times)
        return df.vratiKonacniFlow(), cnt

    FORWARD, BACKWARD = (0, 1), (1, 0)      # a direction: the order in which a pass takes the two images of a level

    def _descend(self, pyramid, dirs, last, bcd_times, coarse_bcd_times, prior_stride, seed_labels, counts, gate=None,
                 gate_bilinear=False):
        """THE coarse-to-fine loop of run, run_pair and coarse_prior: levels len - 1 .. last, each through self.run_level once
        per direction of `dirs`, one prior carried per direction.  Returns the tuple of level 0's flows when last == 0, else the
        tuple of priors of level last - 1 (None without a coarser level).  vratiKonacniFlow returns the level's own buffer, so a
        flow is cloned when, and only when, more than one direction shares the level's DiscreteFlow.  With counts=True an entry
        of self.counts is begun as (level, upsample counts per direction) when the level's priors are made and completed with
        the prior_proposals counts per direction when the level has run; the callers document the rest."""
        priors = (None,) * len(dirs)
        self.counts, self.gate_counts = [], []
        for level in range(len(self.levels) - 1, last - 1, -1):
            flows, cnts = [], []
            for prior, (a, b) in zip(priors, dirs):
                flow, cnt = self.run_level(level, (pyramid[level][a], pyramid[level][b]), bcd_times if level == 0 else coarse_bcd_times,
                                           prior, prior_stride, seed_labels, counts)
                flows.append(flow.clone() if len(dirs) > 1 else flow)
                cnts.append(cnt)
            if counts and priors[0] is not None:
                self.counts[-1] += (tuple(cnts),)
            if level == 0:
                return tuple(flows)
            if gate is not None:
                res = flow_consistency(flows[0], flows[1], gate, bilinear=gate_bilinear, both=True, counts=counts)
                flows = res[:2]
                if counts:
                    self.gate_counts.append((level, res[2]))
            priors = tuple(flow_upsample(f, self.size(level - 1), counts=counts) for f in flows)
            if counts:
                self.counts.append((level - 1, tuple(r[1] for r in priors)))
                priors = tuple(r[0] for r in priors)
        return priors

    def _one_direction(self, res):
        """The edge of a single-direction run: its entry of the tuple `res`, and self.counts' 1-tuples replaced by their tensors."""
        self.counts = [(e[0],) + tuple(t[0] for t in e[1:]) for e in self.counts]
        return res[0]

    def coarse_prior(self, pyramid, bcd_times, prior_stride=2, seed_labels=True, counts=False, gate=None, gate_bilinear=False,
                     pair=False):
        """Levels len - 1 .. 1 run to completion on `pyramid` (image_pyramid), bcd_times sweeps each; returns the upsampled flow of
        level 1, the prior of level 0 ((H,W,3) [U,V,valid]), or None with one level.  With counts=True self.counts is started
        anew and receives one entry (level, int32[3] of flow_upsample, int32[4] of prior_proposals) per coarse level that had a
        prior, and last the entry (0, int32[3] of the upsampling for level 0): the caller that runs level 0's prior step adds its
        counts.  pair=True: the same loop with two directions, every coarse level runs forward and then backward (the images
        swapped), and the pair of priors is returned; the entries of self.counts then hold pairs (forward, backward) in place of
        the tensors.  gate=T (needs pair): the two flows of a coarse level go through flow_consistency(.., T, both=True) before
        they are upsampled, T in pixels of that level; a gated-out vector is invalid, so the finer level's prior step skips what
        the upsampling cannot fill from its neighbours.  With counts=True self.gate_counts holds (level, int32[2,5] of
        flow_consistency) per coarse level."""
        if gate is not None and not pair:
            raise ValueError("PyramidFlow.coarse_prior: gate needs pair=True (the check needs both directions)")
        dirs = (self.FORWARD, self.BACKWARD) if pair else (self.FORWARD,)
        priors = self._descend(pyramid, dirs, 1, None, bcd_times, prior_stride, seed_labels, counts, gate, gate_bilinear)
        return priors if pair else self._one_direction(priors)

    def run_pair(self, pic3, pic4, bcd_times, coarse_bcd_times=None, gate=None, gate_bilinear=False, prior_stride=2, seed_labels=True,
                 counts=False):
        """Both directions of a pair: returns (forward flow, backward flow) of level 0, as tensors of their own.  The image
        pyramid is built once; the loop of run then takes every level forward (pic3 -> pic4) and backward (pic4 -> pic3).
        gate=None: the flows of run(pic3, pic4, ..) and run(pic4, pic3, ..).  gate=T: the two flows of every coarse level go
        through flow_consistency(.., T, both=True[, bilinear=gate_bilinear]) before they are upsampled, so a coarse vector that
        fails the forward/backward check is no prior (coarse_prior; T in pixels of the level it is applied at).  The other
        arguments and self.counts as in run and coarse_prior(pair=True).  With one level these are the calls of two plain runs."""
        if gate is not None:
            gate = float(gate)
            if not (np.isfinite(gate) and gate >= 0):
                raise ValueError("PyramidFlow.run_pair: gate must be None or finite and >= 0, got %r" % gate)
        return self._descend(self.image_pyramid(pic3, pic4), (self.FORWARD, self.BACKWARD), 0, bcd_times,
                             bcd_times if coarse_bcd_times is None else coarse_bcd_times, prior_stride, seed_labels, counts, gate,
                             gate_bilinear)

    def run(self, pic3, pic4, bcd_times, coarse_bcd_times=None, prior_stride=2, seed_labels=True, counts=False):
        """The whole run, one direction; returns level 0's flow tensor (the level's own buffer: nothing is copied).
        coarse_bcd_times: the sweeps of the coarse levels (None: bcd_times).  prior_stride and seed_labels as in
        DiscreteFlow.prior_proposals, for every level that has a prior.  With counts=True self.counts holds, per level that had a
        prior, (level, int32[3] of flow_upsample, int32[4] of prior_proposals) as device tensors.  Everything runs on torch's
        current stream; nothing is read back.  With one level these are exactly the calls of DiscreteFlow.run."""
        return self._one_direction(self._descend(self.image_pyramid(pic3, pic4), (self.FORWARD,), 0, bcd_times,
                                                 bcd_times if coarse_bcd_times is None else coarse_bcd_times, prior_stride,
                                                 seed_labels, counts))
