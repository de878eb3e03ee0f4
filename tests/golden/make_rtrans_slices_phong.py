"""Generates tests/golden/rtrans_slices_phong.npz: rough-transmittance slices (ppg_scene.rtrans layout, 101 floats per case) for the
roughplastic materials with distribution = phong that the tests use, cut from Mitsuba's data/microfacet/phong.dat exactly as
RoughPlastic::configure() does (ppg_host/rtrans.py).  The companion of make_rtrans_slices.py, which covers ggx and beckmann.

Run where a Mitsuba tree is at hand:
    python tests/golden/make_rtrans_slices_phong.py [/path/to/mitsuba/data]
The table is reference *data*; only the slices are stored.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "practical-path-guiding_amd"))
from ppg_host import rtrans  # noqa: E402

# (alpha, eta): eta = polypropylene / air is what a <bsdf type="roughplastic"> without IORs gets
CASES = [("phong", 0.2, float(np.float32(1.49 / 1.000277))), ("phong", 0.2, 1.5)]

if __name__ == "__main__":
    data = sys.argv[1] if len(sys.argv) > 1 else os.environ["PPG_MITSUBA_DATA"]
    out = {"cases": np.array([(d, "%r" % a, "%r" % e) for d, a, e in CASES])}
    for i, (d, a, e) in enumerate(CASES):
        out["slice%d" % i] = rtrans.roughplastic_slice(d, a, e, data)
        assert out["slice%d" % i].shape == (101,)
    np.savez(os.path.join(HERE, "rtrans_slices_phong.npz"), **out)
    print("wrote", os.path.join(HERE, "rtrans_slices_phong.npz"), {k: v.shape for k, v in out.items()})
