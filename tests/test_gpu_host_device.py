"""The image-plane wrappers of pipeline.py take host arrays or device tensors: both give the same bytes, on the current device,
and leave their inputs alone.  9 x 13: H*W is no multiple of the four pixels of a lane.  Run with `pytest -m gpu`."""
import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu

H, W = 9, 13


def inputs():
    rng = np.random.default_rng(11)
    d = dict(bgr=rng.integers(0, 256, (H, W, 3), dtype=np.uint8), img1=rng.integers(0, 256, (H, W, 3), dtype=np.uint8),
             img2=rng.integers(0, 256, (H, W, 3), dtype=np.uint8), edges=rng.random((H, W)).astype(np.float32),
             flow=rng.normal(0, 1.5, (H, W, 2)).astype(np.float32))
    for name, nvalid in (("sparse", 12), ("test", 90), ("gt", 100)):            # [U,V,valid] fields; 12 >= 8 seeds
        f = np.zeros((H * W, 3), np.float32)
        at = rng.choice(H * W, nvalid, replace=False)
        f[at, :2], f[at, 2] = rng.normal(0, 2, (nvalid, 2)), 1
        d[name] = f.reshape(H, W, 3)
    return d


CASES = [("canny_edges", ("bgr",), {}),
         ("pb_edges", ("bgr",), dict(per_orientation=True)),
         ("epic_interpolate", ("sparse", "edges"), dict(nn=4, aux=True)),
         ("epic_prefilter", ("sparse", "edges", "img1"), dict(pref_nn=4, aux=True)),
         ("variational_refine", ("img1", "img2", "flow"), dict(niter_outer=1, niter_solver=2)),
         ("flow_eval", ("test", "gt"), dict(err=True, image=True)),
         ("flow_color", ("flow",), dict(return_radius=True)),
         ("warp_eval", ("img1", "img2", "flow"), dict(warped=True, err=True, image=True))]


@pytest.mark.parametrize("fn,names,kw", CASES, ids=[c[0] for c in CASES])
def test_host_arrays_and_device_tensors_agree(fn, names, kw):
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    dev = torch.device("cuda", torch.cuda.current_device())
    data = inputs()
    host = [data[n].copy() for n in names]
    tensors = [torch.from_numpy(data[n]).to(dev) for n in names]
    runs = []
    for args in (host, tensors):
        out = getattr(pkg("pipeline"), fn)(*args, **kw)
        out = [t for t in (out if isinstance(out, tuple) else (out,)) if t is not None]
        assert all(t.device == dev for t in out)
        runs.append([t.cpu().numpy().tobytes() for t in out])
    assert runs[0] == runs[1] and len(runs[0]) >= 1
    for n, a, t in zip(names, host, tensors):
        assert a.tobytes() == data[n].tobytes() and t.cpu().numpy().tobytes() == data[n].tobytes(), n
