"""Workspaces for tests that check what include/dflow.h promises about d_ws: a stage needs exactly the bytes its size function
names, writes nothing beyond them and reads nothing it has not written.

GuardedWs    one allocation laid out as [front guard | need bytes | back guard]; the region is filled with a poison byte and is
             what the stage gets, the guards must still hold their pattern afterwards.
stage_need   the exact bytes of one entry point for given arguments, from its own DFLOW_ENOSPC message (the public API names only
             the maximum over the main-path stages, dflow_workspace_bytes).  Host only.
guarded      a context manager that makes the pipeline.py wrappers of the image-plane stages draw such workspaces.
guard_pass   the same for a DiscreteFlow.

A plain module: no fixtures, no pytest hooks."""
import contextlib
import ctypes as C
import re

import numpy as np

from conftest import pkg

GUARD = 4096                    # bytes of each guard
GUARD_BYTE = 0xC3               # differs from every poison
POISONS = (0x00, 0xFF, 0x7F)    # zeros; float NaN, int -1, UINT_MAX; a large finite float, a large positive int
PTR = 1 << 20                   # a non-NULL, 1 MiB-aligned stand-in for a device pointer no refused call dereferences
ENOSPC = -2


class GuardedWs:
    """[front guard | need bytes of `poison` | back guard] in one uint8 tensor on `device`.  The region starts `offset` bytes
    after a 256-byte boundary: offset 0 is what every allocator gives, a small offset is the lowest alignment a stage documents."""

    def __init__(self, torch, need, poison, device, offset=0):
        assert need >= 0 and 0 <= offset < 256 and poison != GUARD_BYTE
        self.torch, self.nbytes, self.poison = torch, int(need), poison
        self.buf = torch.full((GUARD + 256 + self.nbytes + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=device)
        self.start = GUARD + (-(self.buf.data_ptr() + GUARD)) % 256 + offset
        self.region = self.buf[self.start:self.start + self.nbytes]
        self.region.fill_(poison)
        self.ptr = self.buf.data_ptr() + self.start
        assert (self.ptr - offset) % 256 == 0 and (self.nbytes == 0 or self.region.data_ptr() == self.ptr)

    def repoison(self):
        self.region.fill_(self.poison)

    def snapshot(self):
        """The region's bytes on the host (waits for the device)."""
        return self.region.cpu().numpy().tobytes()

    def assert_guards(self, what=""):
        """Both guards, and the alignment padding outside them, still hold GUARD_BYTE.  Waits for the device."""
        end = self.start + self.nbytes
        front = np.flatnonzero(self.buf[:self.start].cpu().numpy() != GUARD_BYTE)
        back = np.flatnonzero(self.buf[end:].cpu().numpy() != GUARD_BYTE)
        msg = []
        if front.size:
            msg.append("%d bytes before the workspace changed, offsets %d .. %d from its start"
                       % (front.size, front[0] - self.start, front[-1] - self.start))
        if back.size:
            msg.append("%d bytes after the workspace changed, offsets +%d .. +%d from its end (need %d)"
                       % (back.size, back[0], back[-1], self.nbytes))
        assert not msg, "%s: %s" % (what, "; ".join(msg))


def ws_index(fn_name):
    """The position of d_ws among the arguments of an entry point: the pointer in front of its size_t ws_bytes."""
    argtypes = pkg("_lib")._SIGNATURES[fn_name][1]
    at = [i for i, t in enumerate(argtypes) if t is C.c_size_t]
    assert len(at) == 1 and at[0] >= 1, "%s takes no workspace" % fn_name
    return at[0] - 1


def stage_need(fn_name, *args):
    """The workspace bytes entry point fn_name needs for `args`, its arguments in front of d_ws (device pointers may be PTR:
    nothing is launched).  The call is made with a valid d_ws and ws_bytes = 0 and must answer DFLOW_ENOSPC with CHECK_WS's
    "workspace 0 < N bytes"; anything else is an AssertionError.
    dflow_knn_proposals(_timed) is asked through dflow_knn_screen_stats_n, which checks the same workspace and launches nothing
    whatever the parameters are: where the screened search does not run, dflow_knn_proposals takes no workspace and would run the
    brute-force kernel on these pointers."""
    L = pkg("_lib")
    if fn_name in ("dflow_knn_proposals", "dflow_knn_proposals_timed"):
        assert len(args) == 7, "%s: 7 arguments in front of d_ws, got %d" % (fn_name, len(args))
        fn_name, args, tail = "dflow_knn_screen_stats_n", args[:1], (None, (C.c_int64 * 14)(), 14)
    else:
        i = ws_index(fn_name)
        assert len(args) == i, "%s: %d arguments in front of d_ws, got %d" % (fn_name, i, len(args))
        tail = [None] * (len(L._SIGNATURES[fn_name][1]) - i - 2)     # the stream and whatever follows it
    rc = getattr(L.lib(), fn_name)(*args, PTR, 0, *tail)
    err = L.lib().dflow_last_error().decode()
    m = re.search(r"^dflow_\w+: workspace 0 < (\d+) bytes$", err)
    assert rc == ENOSPC and m, "%s with ws_bytes = 0: expected DFLOW_ENOSPC 'workspace 0 < N bytes', got %d %r" % (fn_name, rc, err)
    return int(m.group(1))


class Handed:
    """What a `guarded` block handed out."""

    def __init__(self):
        self.all = []

    def assert_guards(self, what=""):
        assert self.all, "%s: no workspace was asked for" % what
        for k, g in enumerate(self.all):
            g.assert_guards("%s, workspace %d (%d bytes, poison 0x%02X)" % (what, k, g.nbytes, g.poison))


@contextlib.contextmanager
def guarded(torch, poison, offset=0):
    """Inside the block _lib.workspace, which every image-plane wrapper of pipeline.py asks for its scratch, returns the region
    of a new GuardedWs of exactly the size the stage's size function gives.  Yields the record of what was handed out."""
    L = pkg("_lib")
    real, handed = L.workspace, Handed()

    def workspace(name, h, w, device):
        nbytes = getattr(L.lib(), name)(h, w)
        if nbytes == 0:
            return real(name, h, w, device)                      # the refusal, as it always was
        g = GuardedWs(torch, nbytes, poison, device, offset)
        handed.all.append(g)
        return g.region, nbytes
    L.workspace = workspace
    try:
        yield handed
    finally:
        L.workspace = real


def guard_pass(df, poison, need=None, offset=0):
    """Replaces df.ws / df.ws_bytes of a DiscreteFlow with a guarded region of `need` bytes (default: what it had, the
    dflow_workspace_bytes of its parameters).  Whatever the old workspace held is gone: the BCD records are marked stale."""
    import torch
    g = GuardedWs(torch, df.ws_bytes if need is None else need, poison, df.device, offset)
    df.ws, df.ws_bytes, df._bcd_ready = g.region, g.nbytes, False
    return g
