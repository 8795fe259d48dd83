"""Drop-in for the reference's edge.py: the edge map ivice.bin that spremiZaEpic.py hands to epicflow-static, without cv2.

canny_ivice(fileslike, binfile) reads the image as the first CLI does (PIL -> BGR) and writes (255 - edges) / 255 as raw
float32 (H,W), row-major, no header (edge.py:19-35); the edges come from dflow_canny_edges on the GPU (pipeline.canny_edges).
sed_ivice needs the structured-forest model.yml, which the reference does not ship: it raises.
"""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.basename(os.path.dirname(os.path.abspath(__file__)))

CANNY_LOW, CANNY_HIGH = 100, 200     # edge.py:25


def canny_ivice(fileslike, binfile, low=CANNY_LOW, high=CANNY_HIGH):
    data = canny_ivice_tensor(fileslike, low, high).cpu().numpy()
    with open(binfile, "wb") as f:
        f.write(np.ascontiguousarray(data, dtype=np.float32).tobytes())
    return data


def canny_ivice_tensor(fileslike, low=CANNY_LOW, high=CANNY_HIGH):
    """The (H,W) float32 ivice map of canny_ivice as a device tensor, without writing it."""
    read_bgr = importlib.import_module(PKG + ".daisy i flann").read_bgr
    pipeline = importlib.import_module(PKG + ".pipeline")
    return pipeline.canny_edges(read_bgr(fileslike), low, high, ivice=True)[1]


def sed_ivice(fileslike, binfile):
    raise NotImplementedError("sed_ivice (edge.py:4-17) needs cv2.ximgproc's structured edge detector and its trained "
                              "model.yml, which the reference does not ship; use canny_ivice")
