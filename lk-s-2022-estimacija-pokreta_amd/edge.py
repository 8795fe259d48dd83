"""Drop-in for the reference's edge.py: the edge map ivice.bin that spremiZaEpic.py hands to epicflow-static, without cv2.

canny_ivice(fileslike, binfile) reads the image as the first CLI does (PIL -> BGR) and writes (255 - edges) / 255 as raw
float32 (H,W), row-major, no header (edge.py:19-35); the edges come from dflow_canny_edges on the GPU (pipeline.canny_edges).
sed_ivice needs the structured-forest model.yml, which the reference does not ship: it raises.
pb_ivice(fileslike, binfile, radius) is the model-free substitute for it: it writes 1 - e as raw float32, e the soft edge
strength of dflow_pb_edges (pipeline.pb_edges, DESIGN.md "Pb edge strength"), the file convention of sed_ivice
(edge.py:9,15-16: 1 - the detector's response), so epicflow-static reads it as it would read the sed file.
pb_strength_tensor returns e itself, the strength this package's own interpolation and pre-filter are defined on.
"""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.basename(os.path.dirname(os.path.abspath(__file__)))

CANNY_LOW, CANNY_HIGH = 100, 200     # edge.py:25
PB_RADIUS = 5


def canny_ivice(fileslike, binfile, low=CANNY_LOW, high=CANNY_HIGH):
    data = canny_ivice_tensor(fileslike, low, high).cpu().numpy()
    with open(binfile, "wb") as f:
        f.write(np.ascontiguousarray(data, dtype=np.float32).tobytes())
    return data


def canny_ivice_tensor(fileslike, low=CANNY_LOW, high=CANNY_HIGH):
    """The (H,W) float32 ivice map of canny_ivice as a device tensor, without writing it."""
    read_bgr = importlib.import_module(PKG + ".flowio").read_bgr
    pipeline = importlib.import_module(PKG + ".pipeline")
    return pipeline.canny_edges(read_bgr(fileslike), low, high, ivice=True)[1]


def pb_strength_tensor(fileslike, radius=PB_RADIUS):
    """The (H,W) float32 edge strength e of the image file (dflow_pb_edges) as a device tensor."""
    read_bgr = importlib.import_module(PKG + ".flowio").read_bgr
    pipeline = importlib.import_module(PKG + ".pipeline")
    return pipeline.pb_edges(read_bgr(fileslike), radius)


def write_pb_ivice(strength, binfile):
    """1 - e in float32 of a (H,W) float32 strength (tensor or array) as raw bytes into binfile; returns the array."""
    e = strength.cpu().numpy() if hasattr(strength, "cpu") else np.asarray(strength)
    data = np.ascontiguousarray(np.float32(1.0) - e.astype(np.float32, copy=False), dtype=np.float32)
    with open(binfile, "wb") as f:
        f.write(data.tobytes())
    return data


def pb_ivice(fileslike, binfile, radius=PB_RADIUS):
    return write_pb_ivice(pb_strength_tensor(fileslike, radius), binfile)


def sed_ivice(fileslike, binfile):
    raise NotImplementedError("sed_ivice (edge.py:4-17) needs cv2.ximgproc's structured edge detector and its trained "
                              "model.yml, which the reference does not ship; use canny_ivice")
