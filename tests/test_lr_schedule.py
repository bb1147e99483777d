"""``train.warmup_cosine_lr`` against the learning rates read from a real ``torch.optim.Adam`` under the reference's scheduler pair
(tests/golden/lr_schedule.json, written by tools/make_train_fixtures.py): epochs = 60, every epoch 0..60, and epochs = 3000, epochs
0..40, 1500 and 3000.  Relative 1e-9: the reference updates the cosine part recursively, at most 3000 double-precision
updates of relative error 1e-16 each stay below 1e-12, so the bound is margin, not slack."""
import json
import os

import cases  # noqa: F401  (puts the repository on sys.path)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lr_schedule.json")


def test_schedule_matches_the_recorded_optimizer():
    from bayer_low_light_image_enhancement_amd.train import warmup_cosine_lr
    fx = json.load(open(GOLDEN))
    assert [r["epochs"] for r in fx["runs"]] == [60, 3000]
    assert sorted(int(e) for e in fx["runs"][0]["lr"]) == list(range(61))
    assert sorted(int(e) for e in fx["runs"][1]["lr"]) == list(range(41)) + [1500, 3000]
    for run in fx["runs"]:
        for e, want in run["lr"].items():
            got = warmup_cosine_lr(int(e), fx["base_lr"], run["epochs"], fx["warmup"], fx["eta_min"])
            assert abs(got - want) <= 1e-9 * abs(want), (run["epochs"], e, got, want)


def test_epoch_zero_trains_at_exactly_zero():
    from bayer_low_light_image_enhancement_amd.train import warmup_cosine_lr
    fx = json.load(open(GOLDEN))
    for run in fx["runs"]:
        assert run["lr"]["0"] == 0.0
        assert warmup_cosine_lr(0, fx["base_lr"], run["epochs"], fx["warmup"], fx["eta_min"]) == 0.0
    assert warmup_cosine_lr(0) == 0.0


def test_hand_over_quirks():
    """Full rate at the end of the ramp, ABOVE it for the one epoch in which the un-stepped cosine scheduler takes over, back at
    it in the next; the defaults are the reference's."""
    from bayer_low_light_image_enhancement_amd.train import warmup_cosine_lr
    assert warmup_cosine_lr(20) == 1e-4
    assert warmup_cosine_lr(21) > 1e-4 and warmup_cosine_lr(21, epochs=60) > warmup_cosine_lr(21)
    assert abs(warmup_cosine_lr(22) - 1e-4) <= 1e-19
    assert warmup_cosine_lr(3000) > 1e-5
