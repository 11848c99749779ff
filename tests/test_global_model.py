"""The model of the registration without a start pose (tests/global_ref.py) against what include/smx.h states, without a GPU: the
lattice's counts, order and rotations; the recorded words of tests/golden/global_bracket.npz against the model they were taken
from; the model's end-to-end run on the bracket against the TRUE pose; and every mutant of the model against a named case."""
import numpy as np
import pytest

import global_ref as gr
import register_ref as rr
import track_ref as tr


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_the_lattice_is_what_the_contract_says(k):
    q = gr.quaternions(k)
    assert q.shape[0] == gr.n_rotations(k) == ((2 * k + 1) ** 4 - (2 * k - 1) ** 4) // 2 == (40, 272, 888, 2080)[k - 1]
    # the order: ascending lexicographic (w, x, y, z); the largest component, the sign
    rows = [tuple(r) for r in q.tolist()]
    assert rows == sorted(rows) and len(set(rows)) == len(rows)
    assert np.all(np.abs(q).max(axis=1) == k)
    first = np.array([next(v for v in r if v != 0) for r in rows])
    assert np.all(first > 0)
    assert (k, 0, 0, 0) in rows
    R = gr.rotations(k)
    assert np.array_equal(R[rows.index((k, 0, 0, 0))], np.eye(3))
    eye = np.einsum("nij,nkj->nik", R, R)
    assert np.abs(eye - np.eye(3)).max() <= 1e-15, np.abs(eye - np.eye(3)).max()
    assert np.abs(np.linalg.det(R) - 1.0).max() <= 1e-14
    # no two parallel: no rotation repeats
    unit = q / np.linalg.norm(q, axis=1, keepdims=True)
    dots = np.abs(unit @ unit.T) - np.eye(q.shape[0])
    assert dots.max() < 1.0 - 1e-9, dots.max()
    assert np.unique(R.reshape(-1, 9).round(12), axis=0).shape[0] == q.shape[0]


def test_the_poses_of_the_lattice_and_their_order():
    c, a = np.array([0.3, -0.2, 0.7]), np.array([[1.0, 2.0, 3.0], [-0.5, 0.25, 0.125]])
    poses = gr.lattice(2, c, a)
    R = gr.rotations(2)
    assert poses.shape == (272 * 2, 3, 4) and poses.dtype == np.float32
    for i in (0, 1, 77, 271):
        for j in (0, 1):
            P = poses[i * 2 + j].astype(np.float64)
            assert np.array_equal(P[:, :3], R[i].astype(np.float32).astype(np.float64))
            # the centre lands on the anchor
            assert np.allclose(R[i] @ c + (a[j] - R[i] @ c), a[j], atol=1e-15) and np.allclose(P[:, :3] @ c + P[:, 3], a[j], atol=1e-6)


# The largest angle from a rotation to the nearest rotation of the lattice over 2000 seeded uniformly random rotations, measured
# here (numpy, default_rng(7)): MAXIMA OF A SAMPLE, no bounds -- another sample gives another few degrees (DESIGN.md 5s quotes both
# this sample and the one the feature was proposed with).
COVERAGE_DEG = {1: 59.96, 2: 38.94, 3: 26.03, 4: 21.23, 5: 16.51, 6: 14.44}


def test_the_coverage_of_the_lattice_is_measured():
    rng = np.random.default_rng(7)
    Rs = [gr.random_rotation(rng) for _ in range(2000)]
    for k, want in COVERAGE_DEG.items():
        got = max(gr.nearest_lattice_angle_deg(k, R)[0] for R in Rs)
        print("k = %d: %d rotations, the farthest of 2000 sampled rotations lies %.2f degrees from the nearest" % (k, gr.n_rotations(k), got))
        assert abs(got - want) < 0.05, (k, got, want)


def test_the_recorded_words_are_the_models():
    """tests/golden/global_bracket.npz against the model it was taken from (the slow half of this file: brute force)."""
    for seed in gr.BRACKET_SEEDS:
        want = gr.score(gr.bracket_mesh(), gr.bracket_points(seed)[0], gr.bracket_poses(seed, 3), 1, gr.BRACKET_BOUND)
        assert gr.golden_scores(seed).tobytes() == want.tobytes(), seed
    for name in gr.cases():
        for q in gr.gates_of(name):
            assert gr.golden_case(name, q).tobytes() == gr.model_scores(name, q).tobytes(), (name, q)


# The model's own distance from the true pose on the bracket (k = 3, one centroid anchor, gate 0.05 m, 8 starts, the default
# schedule), measured on the CPU -- the restatement's own chain in double, no device in it: at most 1.1e-7 rad and 1.4e-7 m over
# the three seeds (the samples lie on the triangles up to their rounding to float32, a metre from the origin).  Asserted with a
# 4x margin, on the CPU model against the truth, never on the device against itself.  The candidate nearest the truth ranked
# 0, 0 and 1 by cost: asserted as at most 1.
BRACKET_MODEL_ROTATION, BRACKET_MODEL_TRANSLATION, BRACKET_MODEL_RANK = 1.1e-7, 1.4e-7, 1


@pytest.mark.parametrize("seed", gr.BRACKET_SEEDS)
def test_the_model_finds_the_bracket_from_nowhere(seed):
    pts, nrm, T_true = gr.bracket_points(seed)
    poses = gr.bracket_poses(seed, 3)
    scores = gr.golden_scores(seed)
    angle, nearest = gr.nearest_lattice_angle_deg(3, T_true)
    order = gr.select(scores["cost"], poses.shape[0])
    rank = int(np.flatnonzero(order == nearest)[0])
    g = gr.register_global(gr.bracket_mesh(), pts, nrm, poses, rr.Params(), gr.BRACKET_BOUND, scores=scores)
    dt, dr_ = tr.pose_difference(g["T"].astype(np.float64), T_true)
    print("seed %d: the truth turns by %.1f degrees; the nearest candidate (%.1f degrees off) ranks %d; winner rank %d, %.3g rad and %.3g m "
          "from the truth; cost %s -> %s" % (seed, gr.rotation_angle_deg(T_true, np.eye(3)), angle, rank, g["winner_rank"], dr_, dt,
                                             scores["cost"][g["order"]].tolist(), g["after"]["cost"].tolist()))
    assert rank <= BRACKET_MODEL_RANK, rank
    assert g["found"] and g["calls"][g["winner_rank"]]["status"] in (tr.OK, tr.CONVERGED)
    assert dr_ <= 4 * BRACKET_MODEL_ROTATION and dt <= 4 * BRACKET_MODEL_TRANSLATION, (dr_, dt)


def test_a_rotation_above_ninety_degrees_is_among_the_seeds():
    assert max(gr.rotation_angle_deg(gr.bracket_points(s)[2], np.eye(3)) for s in gr.BRACKET_SEEDS) > 90.0


def test_every_mutant_changes_a_word_of_a_named_case():
    world, q = "base set, k = 1 about its pose, stride 3", 0.02
    base = gr.model_scores(world, q)
    seen = {}
    for mutant in ("unmatched_free", "bad_free", "stride_plus_one"):
        got = gr.model_scores(world, q, mutant)
        words = [w for w in ("cost", "n_ok", "n_matched", "n_rim") if not np.array_equal(got[w], base[w])]
        seen[mutant] = (world, words)
    # the order of the poses: two anchors
    c, a = np.array([0.3, -0.2, 0.7]), np.array([[1.0, 2.0, 3.0], [-0.5, 0.25, 0.125]])
    seen["anchor_major"] = ("the k = 1 lattice on two anchors", ["poses"] if gr.lattice(1, c, a, "anchor_major").tobytes() != gr.lattice(1, c, a).tobytes() else [])
    # a tie: a pose given twice
    cost = np.concatenate([base["cost"], base["cost"][:5]])
    seen["tie_later"] = ("the base set's poses with the first five given again", ["order"] if not np.array_equal(gr.select(cost, 8, "tie_later"), gr.select(cost, 8)) else [])
    # the winner: seed 3, whose cheapest start fails and keeps its cost
    pts, nrm, _ = gr.bracket_points(3)
    args = (gr.bracket_mesh(), pts, nrm, gr.bracket_poses(3, 3), rr.Params(), gr.BRACKET_BOUND)
    own, mut = gr.register_global(*args, scores=gr.golden_scores(3)), gr.register_global(*args, scores=gr.golden_scores(3), mutant="winner_before")
    seen["winner_before"] = ("the bracket, seed 3", ["winner_rank"] if own["winner_rank"] != mut["winner_rank"] else [])
    for mutant, (case, words) in seen.items():
        print("%s (%s) -> %s: %s" % (mutant, gr.MUTANTS[mutant], case, ", ".join(words) or "NOTHING"))
    assert set(seen) == set(gr.MUTANTS)
    assert all(words for _, words in seen.values()), seen
