"""What rim rejection and robust weights are for, asserted on the exact model on the CPU (tests/register_robust_ref.py), never on
the device: a patch cut out of a larger curved surface, registered from points that cover the whole surface (a partial overlap),
and from points of the patch of which 15 % are lifted off it (one-sided outliers).  MEASURED holds the distances from the true
pose that the model's own chain reaches (default schedule, no normals; written down in DESIGN.md 5r); every value has to come
out within a factor of 4 of what is written here, and every robust variant has to end nearer to the truth than the plain call on
the same points.  The device is held to the model, bit for bit, by tests/test_gpu_register_robust.py."""
import pytest

import register_robust_ref as rb
import track_ref as tr

# (variant, bound) -> translation error in metres
MEASURED = {
    ("plain", 0.02): 3.5e-4, ("plain", 0.05): 1.8e-3,
    ("rim rejected", 0.02): 1.0e-8, ("rim rejected", 0.05): 1.0e-8,
    ("rim + Tukey 16 / 8 / 4 mm", 0.02): 2.0e-8, ("rim + Tukey 16 / 8 / 4 mm", 0.05): 2.0e-8,
    ("outliers, plain", 0.02): 2.6e-3, ("outliers, Huber 2 mm", 0.02): 7.1e-4, ("outliers, Tukey 4 mm", 0.02): 1.1e-6,
}
BETTER = (("rim rejected", "plain", 0.02), ("rim rejected", "plain", 0.05), ("rim + Tukey 16 / 8 / 4 mm", "plain", 0.02),
          ("rim + Tukey 16 / 8 / 4 mm", "plain", 0.05), ("outliers, Huber 2 mm", "outliers, plain", 0.02),
          ("outliers, Tukey 4 mm", "outliers, Huber 2 mm", 0.02))


def test_the_fixture_is_what_it_says():
    f = rb.patch()
    assert 1000 <= f["mesh"].tri.shape[0] <= 1100 and f["whole"].shape == (3000, 3) and f["inner"].shape == (3000, 3)
    assert 400 <= f["n_lifted"] <= 500
    rim = rb.rim_of(f["mesh"])
    assert 100 < int((rim != 0).sum()) < 400          # the patch has a rim, and an interior


@pytest.mark.parametrize("key", list(MEASURED), ids=lambda k: "%s at %g" % k)
def test_every_variant_ends_where_it_was_measured(key):
    call, dt, drot = rb.patch_call(*key)
    print("%s at %g: %.3g m and %.3g rad from the truth after %d iterations, status %d" % (key[0], key[1], dt, drot, call["iterations_run"], call["status"]))
    assert call["status"] in (tr.OK, tr.CONVERGED)
    assert MEASURED[key] / 4 <= dt <= MEASURED[key] * 4, (key, dt)


@pytest.mark.parametrize("robust, plain, bound", BETTER)
def test_the_robust_variant_ends_nearer_to_the_truth(robust, plain, bound):
    assert rb.patch_call(robust, bound)[1] < rb.patch_call(plain, bound)[1]


def test_what_the_counts_say_on_the_patch():
    """A larger gate lets more samples beyond the edge find the rim; Tukey at 4 mm rejects nearly every lifted point and hardly
    another."""
    near, far = (rb.patch_call("rim rejected", b)[0]["records"][-1]["sums"] for b in (0.02, 0.05))
    assert 0 < near[rb.S_RIM] < far[rb.S_RIM] and near[28] == far[28]                  # the same inliers at both gates
    last = rb.patch_call("outliers, Tukey 4 mm", 0.02)[0]["records"][-1]["sums"]
    lifted = rb.patch()["n_lifted"]
    assert lifted - 10 <= last[rb.S_WEIGHT] <= lifted + 10
