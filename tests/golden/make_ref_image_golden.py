#!/usr/bin/env python
"""Generates tests/golden/ref_image_fns.npz: the inputs of tests/test_oracle_ref_image_pin.py and the REFERENCE's outputs
on them -- its three input-side image functions, run from oracle/_ref/libsmx_ref_image.so (oracle/ref_build.py compiles
them from the reference's text where the reference sources are at hand).  Recorded results only: no program text.

    python oracle/ref_build.py && python tests/golden/make_ref_image_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import test_oracle_ref_image_pin as pin  # noqa: E402

if __name__ == "__main__":
    if not os.path.exists(pin.SO):
        sys.exit("%s is not built (python oracle/ref_build.py, with the reference sources at hand)" % pin.SO)
    g = pin.record(pin.RefImageFns(pin.SO))
    np.savez_compressed(pin.GOLDEN, **g)
    print("%s: %d arrays, %d bytes" % (os.path.relpath(pin.GOLDEN), len(g), os.path.getsize(pin.GOLDEN)))
