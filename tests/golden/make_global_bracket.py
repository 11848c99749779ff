#!/usr/bin/env python
"""Generates tests/golden/global_bracket.npz: the words of the CPU model of tests/global_ref.py for the end-to-end cases of the
registration without a start pose -- per seed of global_ref.BRACKET_SEEDS the 888 pose scores of the k = 3 lattice on the
bracket (stride 1, gate 0.05 m), which take the brute-force model ten seconds a seed, and the scores of every case of
global_ref.cases() at every gate it runs at.  Recorded results only;
tests/test_global_model.py checks the file against the model, the GPU tests read it.

    python tests/golden/make_global_bracket.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import global_ref as gr  # noqa: E402

if __name__ == "__main__":
    out = {}
    for seed in gr.BRACKET_SEEDS:
        pts = gr.bracket_points(seed)[0]
        sc = gr.score(gr.bracket_mesh(), pts, gr.bracket_poses(seed, 3), 1, gr.BRACKET_BOUND)
        for name in ("cost", "n_ok", "n_matched", "n_rim"):
            out["%s_%d" % (name, seed)] = sc[name]
    for case in gr.cases():                             # (the world's brute force takes its half minute too)
        for q in gr.gates_of(case):
            sc = gr.model_scores(case, q)
            for name in ("cost", "n_ok", "n_matched", "n_rim"):
                out["%s|%s|%g" % (name, case, q)] = sc[name]
    path = os.path.join(HERE, gr.GOLDEN)
    np.savez_compressed(path, **out)
    print("%s: %d arrays, %d bytes" % (os.path.relpath(path), len(out), os.path.getsize(path)))
