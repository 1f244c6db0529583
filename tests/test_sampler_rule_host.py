"""
The train sampler's accept / reject rule against the reference's own behaviour: tests/golden/sampler_rule_golden.json
holds, per scenario, a scripted table of candidates per (slot, try) and the try at which the unmodified
IsotrophicLiveViewSequence2D accepted each slot (oracle/gen_golden_sampler.py). Both the plain restatement
(tests/sampler_ref.py) and data.SliceRule, which TrainSampler uses for every decision, must reproduce every slot.
"""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_ref                                                                      # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampler_rule_golden.json")
HAND_WRITTEN = ("last_slot_demands_all_classes", "kept_after_allbg_rejection", "tenth_try_unconditional",
                "one_class_fg_is_label_1", "auto_resolves_to_no_forcing", "labels_beyond_n_classes",
                "label_32_and_up_is_no_class", "fraction_zero", "fraction_one")


@pytest.fixture(scope="module")
def scenarios():
    with open(GOLDEN) as f:
        return json.load(f)


def _mask(classes):
    m = 0
    for c in classes:
        if c < 32:                                            # what mpu_plane_stats reports: labels < 32
            m |= 1 << c
    return m


def _rule_tries(sc):
    from multiplanarunet_amd.data import SliceRule
    rule = SliceRule(sc["batch_size"], sc["n_classes"], sc["fg_batch_fraction"], sc["force_all_fg"], max_tries=10)
    out = []
    for slot, row in enumerate(sc["table"]):
        for t, (classes, flag) in enumerate(row, 1):
            if rule.judge(slot, t, _mask(classes), bool(flag)):
                out.append(t)
                break
        else:
            out.append(None)
    return out


def test_golden_covers_the_ranges_and_the_hand_written_cases(scenarios):
    names = {sc["name"] for sc in scenarios}
    assert all(n in names for n in HAND_WRITTEN)
    rnd = [sc for sc in scenarios if sc["name"].startswith("random_")]
    assert len(rnd) >= 300
    assert {sc["batch_size"] for sc in rnd} >= {1, 2, 16} and {sc["n_classes"] for sc in rnd} >= {1, 2, 3, 16}
    assert {sc["fg_batch_fraction"] for sc in rnd} == {0.0, 0.25, 0.5, 1.0}
    assert {str(sc["force_all_fg"]) for sc in rnd} == {"auto", "True", "False"}
    assert any(c >= sc["n_classes"] for sc in rnd for row in sc["table"] for cl, _ in row for c in cl)
    assert any(c >= 32 for sc in scenarios for row in sc["table"] for cl, _ in row for c in cl)
    for sc in scenarios:
        assert len(sc["table"]) == sc["batch_size"] == len(sc["accepted_try"])
        assert all(len(row) == 10 for row in sc["table"]) and all(1 <= t <= 10 for t in sc["accepted_try"])
    tries = [t for sc in scenarios for t in sc["accepted_try"]]
    assert 1 in tries and 10 in tries and any(1 < t < 10 for t in tries)


def test_restatement_reproduces_the_reference_on_every_slot(scenarios):
    bad = [sc["name"] for sc in scenarios
           if sampler_ref.accepted_tries([[(cl, bool(f)) for cl, f in row] for row in sc["table"]], sc["batch_size"],
                                         sc["n_classes"], sc["fg_batch_fraction"], sc["force_all_fg"]) != sc["accepted_try"]]
    assert not bad, "%d of %d scenarios differ: %s" % (len(bad), len(scenarios), bad[:5])


def test_slice_rule_reproduces_the_reference_on_every_slot(scenarios):
    """Fails on a rule that carries the classes-seen mask across slots and updates it on acceptance only (the sampler before
    SliceRule): 64 of the 320 scenarios then differ from the reference, 8 of the 20 hand-written ones among them."""
    bad = [(sc["name"], _rule_tries(sc), sc["accepted_try"]) for sc in scenarios if _rule_tries(sc) != sc["accepted_try"]]
    assert not bad, "%d of %d scenarios differ, first: %s" % (len(bad), len(scenarios), bad[0])


def test_slice_rule_keeps_has_fg_over_the_batch_and_resets(scenarios):
    from multiplanarunet_amd.data import SliceRule
    rule = SliceRule(4, 3, 0.5, "auto", 10)
    assert rule.fg_classes == [1, 2] and rule.n_fg_slices == 2 and rule.force_all_fg is True
    assert SliceRule(2, 3).force_all_fg is False and SliceRule(2, 1).fg_classes == [1] and SliceRule(3, 3, 0.4).n_fg_slices == 2
    assert rule.judge(0, 1, 0b010, True) and rule.has_fg == 1
    assert rule.judge(1, 1, 0b001, True) and rule.has_fg == 1
    rule.reset()
    assert rule.has_fg == 0
    # max_tries below the reference's 10: the last try is the unconditional one
    r3 = SliceRule(1, 3, 1.0, "auto", 3)
    assert [r3.judge(0, t, 0, False) for t in (1, 2, 3)] == [False, False, True]
