"""
TEST INFRASTRUCTURE ONLY -- generates tests/golden/sampler_rule_golden.json by running the reference's own, unmodified
training sequence (mpunet/sequences/isotrophic_live_view_sequence_2d.py `IsotrophicLiveViewSequence2D.__getitem__` /
`_get_valid_slice_from`, with `validate_lab_vec`, `validate_lab`, `is_valid_im` of isotrophic_live_view_sequence.py) on
a fake image-pair queue whose interpolator returns SCRIPTED planes. Run by hand where the reference exists:

    PYTHONDONTWRITEBYTECODE=1 python oracle/gen_golden_sampler.py

A script entry is (class list, not-all-background flag) per (slot, try): the label plane holds exactly those labels (and
0), the image plane is the constant bg_value plus one altered pixel when the flag is set. The queue's get_random_image
context is where a new slot starts; the number of label planes the reference asked for inside one context is the try at
which that slot was accepted. The file holds only data: per scenario the settings, the batch_size x 10 table (flag as
0 / 1) and the accepted try per slot.
"""
import contextlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_shim  # noqa: E402

ref_shim.install()
from mpunet.sequences.isotrophic_live_view_sequence_2d import IsotrophicLiveViewSequence2D  # noqa: E402

DIM, MAX_TRIES = 8, 10                                        # (max_tries is a literal 10 in the reference's __getitem__)


class ScriptedInterpolator:
    bg_value = [0.5]

    def __init__(self, table):
        self.table, self.slot, self.t, self.flag = table, -1, 0, 0

    def intrp_labels(self, grid):
        classes, self.flag = self.table[self.slot][self.t]
        self.t += 1
        lab = np.zeros((DIM, DIM), np.uint8)
        for k, c in enumerate(classes):
            lab[1 + k // DIM, k % DIM] = c
        return lab

    def intrp_image(self, grid):
        im = np.full((DIM, DIM, 1), self.bg_value[0], np.float32)
        if self.flag:
            im[1, 1, 0] += 1.0
        return im


class IdentityScaler:
    @staticmethod
    def transform(x):
        return x


class FakeImage:
    sample_weight = 1.0
    scaler = IdentityScaler

    def __init__(self, table):
        self.interpolator = ScriptedInterpolator(table)


class FakeQueue:
    def __init__(self, image):
        self.image, self.accepted = image, []

    @contextlib.contextmanager
    def get_random_image(self):
        it = self.image.interpolator
        it.slot += 1
        it.t = 0
        yield self.image
        self.accepted.append(it.t)


def run_reference(sc):
    queue = FakeQueue(FakeImage(sc["table"]))
    seq = IsotrophicLiveViewSequence2D(queue, views=np.eye(3), no_log=True, dim=DIM, batch_size=sc["batch_size"],
                                       n_classes=sc["n_classes"], real_space_span=float(DIM), noise_sd=0.1,
                                       fg_batch_fraction=sc["fg_batch_fraction"], force_all_fg=sc["force_all_fg"],
                                       logger=lambda *a, **k: None)
    seq.seed = lambda: None
    np.random.seed(0)                                         # (the plane geometry is drawn and ignored)
    seq[0]
    assert len(queue.accepted) == sc["batch_size"]
    return queue.accepted


def scenario(name, B, K, table, frac=0.5, force="auto"):
    assert len(table) == B and all(len(r) == MAX_TRIES for r in table), name
    return {"name": name, "batch_size": B, "n_classes": K, "fg_batch_fraction": frac, "force_all_fg": force,
            "table": [[[sorted(int(c) for c in cl), int(bool(f))] for cl, f in row] for row in table]}


def rows(*specs, fill=((), 1)):
    """One table row: the given entries, padded to MAX_TRIES with `fill`."""
    r = [(tuple(c), f) for c, f in specs]
    return r + [fill] * (MAX_TRIES - len(r))


def hand_written():
    E, out = ((), 1), []
    # the last slot demands all classes: B=4, K=3; slot 3 has one slice left, so both classes must have been seen IN THIS SLOT
    out.append(scenario("last_slot_demands_all_classes", 4, 3,
                        [rows(([1], 1)), rows(([2], 1)), rows(([1, 2], 1)),
                         rows(([1], 1), ([], 1), ([1], 1), ([1, 2], 1), ([2], 1))]))
    # ... and earlier slots' classes do not count for it; the slot before wants at least one class
    out.append(scenario("classes_of_earlier_slots_do_not_count", 3, 3,
                        [rows(([1, 2], 1)), rows(([], 1), ([2], 1)), rows(([1], 1), ([2], 1), ([1], 1), ([2, 1], 1))]))
    # single classes seen in tries the vector check rejects never add up (the vector is rebound only on a pass)
    out.append(scenario("rejected_tries_do_not_accumulate", 3, 3,
                        [rows(([1], 1)), rows(([2], 1)), rows(([1], 1), ([2], 1), ([1], 1), ([2], 1), ([1, 2], 1))]))
    # passes the vector check, rejected as all-background: its classes count for the next try of the slot, here an empty plane
    out.append(scenario("kept_after_allbg_rejection", 3, 3,
                        [rows(([1], 1)), rows(([1], 1)), rows(([1, 2], 0), ([], 1))]))
    out.append(scenario("kept_after_allbg_rejection_then_fraction", 4, 3,
                        [rows(([], 1)), rows(([], 1)), rows(([1], 0), ([], 1), ([2], 1)),
                         rows(([1, 2], 0), ([], 1), ([], 0), ([2], 1))], frac=1.0))
    # passes the vector check, rejected by the foreground fraction; in the last slot class 1, kept from an all-background
    # plane, lets an empty plane pass the vector check, which the fraction then rejects
    out.append(scenario("fraction_rejection_after_vector_pass", 4, 2,
                        [rows(([], 1)), rows(([], 1)), rows(([], 1), ([1], 1)), rows(([1], 0), ([], 1), ([1], 1))]))
    # the tenth try is accepted unconditionally: no foreground, all background, vector check skipped
    out.append(scenario("tenth_try_unconditional", 2, 3, [rows(fill=((), 0)), rows(fill=((), 0))]))
    out.append(scenario("tenth_try_unconditional_fg_counts", 3, 2,
                        [rows(*[([1], 0)] * 10), rows(fill=((), 0)), rows(fill=((), 1))], frac=1.0))
    out.append(scenario("tenth_try_skips_vector_check", 1, 4, [rows(*[([1], 1)] * 10)], force=True))
    # K=1: fg_classes is [1]
    out.append(scenario("one_class_fg_is_label_1", 4, 1,
                        [rows(([], 1)), rows(([], 1)), rows(([], 1), ([2], 1), ([1], 1)), rows(([], 1), ([1], 0), ([1], 1))]))
    out.append(scenario("one_class_last_slot", 2, 1, [rows(([0], 1)), rows(([], 1), ([3], 1), ([1], 1))], frac=0.0))
    # B <= number of foreground classes: auto resolves to no forcing
    out.append(scenario("auto_resolves_to_no_forcing", 3, 4,
                        [rows(([], 1)), rows(([], 1), ([1], 1)), rows(([], 1), ([], 1), ([3], 0), ([2], 1))]))
    out.append(scenario("same_table_forced_on", 3, 4,
                        [rows(([], 1)), rows(([], 1), ([1], 1)), rows(([], 1), ([], 1), ([3], 0), ([2], 1))], force=True))
    out.append(scenario("auto_boundary_b_equals_nfg_plus_1", 4, 4,
                        [rows(([], 1)), rows(([], 1), ([1], 1)), rows(([2], 1)), rows(([1, 2], 1), ([1, 2, 3], 1))]))
    # labels >= n_classes and a label >= 32
    out.append(scenario("labels_beyond_n_classes", 4, 3,
                        [rows(([3], 1)), rows(([7, 31], 1)), rows(([3, 7], 1), ([32], 1), ([2], 1)),
                         rows(([1, 40], 1), ([34, 33], 1), ([1, 2, 255], 1))]))
    out.append(scenario("label_32_and_up_is_no_class", 2, 16,
                        [rows(([32, 33, 64, 255], 1)), rows(([32 + c for c in range(1, 16)], 1), (list(range(1, 16)), 1))]))
    # fg_batch_fraction 0 and 1
    out.append(scenario("fraction_zero", 4, 3, [rows(E), rows(E), rows(E), rows(E, ([1], 1), ([1, 2], 1))], frac=0.0))
    out.append(scenario("fraction_zero_no_forcing", 4, 3, [rows(E), rows(E), rows(E), rows(E)], frac=0.0, force=False))
    out.append(scenario("fraction_one", 4, 3,
                        [rows(E, ([1], 1)), rows(E, E, ([2], 0), ([2], 1)), rows(([1], 1)), rows(([1], 1), ([2, 1], 1))],
                        frac=1.0))
    out.append(scenario("fraction_one_no_forcing", 3, 3,
                        [rows(E, ([1], 1)), rows(E, E, ([2], 0), ([2], 1)), rows(fill=((), 1))], frac=1.0, force=False))
    return out


def random_scenarios(n=300, seed=2):
    rng = np.random.RandomState(seed)
    out = []
    for i in range(n):
        B = int(rng.choice([1, 2, 2, 3, 4, 6, 8, 16]))
        K = int(rng.choice([1, 2, 3, 4, 5, 8, 16]))
        frac = float(rng.choice([0.0, 0.25, 0.5, 1.0]))
        force = ["auto", True, False][rng.randint(3)]
        p_fg, p_nonbg = rng.choice([0.05, 0.4, 0.8]), rng.choice([0.5, 0.95])
        hi = K + 2 if rng.rand() < 0.8 else 40                # mostly labels up to n_classes + 1, sometimes up to 39
        table = [[(sorted(set(int(c) for c in rng.randint(1, hi, rng.randint(1, 5)))) if rng.rand() < p_fg else [],
                   bool(rng.rand() < p_nonbg)) for _ in range(MAX_TRIES)] for _ in range(B)]
        out.append(scenario("random_%03d" % i, B, K, table, frac, force))
    return out


def main():
    out = hand_written() + random_scenarios()
    for sc in out:
        sc["accepted_try"] = run_reference(sc)
    dst = os.path.join(HERE, "..", "tests", "golden", "sampler_rule_golden.json")
    with open(dst, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(sc, separators=(",", ":")) for sc in out) + "\n]\n")
    for sc in out[:len(hand_written())]:
        print(sc["name"], sc["accepted_try"])
    print(len(out), "scenarios,", os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
