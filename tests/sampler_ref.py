"""
Plain-Python restatement of the accept / reject rule of the reference's training sequence, over class SETS:
`_get_valid_slice_from` (mpunet/sequences/isotrophic_live_view_sequence_2d.py:119-161) with `validate_lab_vec`,
`validate_lab` and `is_valid_im` (isotrophic_live_view_sequence.py:91-128). Independent of data.SliceRule (no bit masks,
no shared code); tests/golden/sampler_rule_golden.json, recorded from the reference class itself, pins both.

What the reference really does, and a reader does not expect: `validate_lab_vec` returns a NEW array and
`_get_valid_slice_from` rebinds only its local name, so the "classes seen" vector that `__getitem__` passes in is all
zero for EVERY slot of a batch; it accumulates over the tries of that one slot only, and keeps the classes of a candidate
that passed the vector check even when `validate_lab` or `is_valid_im` then rejects that candidate.
"""
import math


def settings(batch_size, n_classes, fg_batch_fraction=0.5, force_all_fg="auto"):
    """(fg classes, n_fg_slices, forcing on) as the reference's properties resolve them."""
    fg_classes = list(range(1, n_classes)) or [1]
    n_fg_slices = int(math.ceil(batch_size * fg_batch_fraction))
    if isinstance(force_all_fg, str) and force_all_fg.lower() == "auto":
        forcing = batch_size > len(fg_classes)
    else:
        forcing = bool(force_all_fg)
    return fg_classes, n_fg_slices, forcing


def slot_tries(candidates, slot, has_fg_count, batch_size, n_classes, fg_batch_fraction=0.5, force_all_fg="auto",
               max_tries=10):
    """Judge the candidates of ONE slot in order. candidates: sequence of (classes, nonbg) -- the labels present in the
    plane (any iterable of ints; 0 and labels that are no foreground class are ignored) and whether the image plane is not
    all background. Returns (accepted try, 1-based, or None if the sequence ran out first; the slot's foreground count 0/1;
    per try one of 'vec' / 'fraction' / 'allbg' / 'accept' / 'forced'; per try whether its classes entered the slot's
    vector)."""
    fg_classes, n_fg_slices, forcing = settings(batch_size, n_classes, fg_batch_fraction, force_all_fg)
    left = batch_size - slot
    seen = {c: 0 for c in fg_classes}                         # has_fg_vec: zeros for every slot
    verdicts, kept = [], []
    for t, (classes, nonbg) in enumerate(candidates, 1):
        if t > max_tries:
            break
        classes = set(int(c) for c in classes)
        last = t == max_tries
        took = False
        if forcing and not last:
            new = {c: seen[c] + (1 if c in classes else 0) for c in fg_classes}
            n_missing = sum(1 for c in fg_classes if new[c] == 0)
            if not (n_missing == 0 or n_missing < left):
                verdicts.append("vec"); kept.append(False)
                continue
            seen, took = new, True                            # stays, whatever the two checks below say
        kept.append(took)
        vec_would_pass = True                                 # (only to name a last-try acceptance 'forced'; decides nothing)
        if forcing and last:
            n_missing = sum(1 for c in fg_classes if seen[c] == 0 and c not in classes)
            vec_would_pass = n_missing == 0 or n_missing < left
        if any(c in classes for c in fg_classes):
            valid, change = True, 1
        elif n_fg_slices - has_fg_count < left:
            valid, change = True, 0
        else:
            valid, change = False, 0
        if not (valid or last):
            verdicts.append("fraction")
            continue
        if last or nonbg:
            verdicts.append("forced" if last and not (valid and nonbg and vec_would_pass) else "accept")
            return t, change, verdicts, kept
        verdicts.append("allbg")
    return None, 0, verdicts, kept


def accepted_tries(table, batch_size, n_classes, fg_batch_fraction=0.5, force_all_fg="auto", max_tries=10):
    """The try (1-based) at which each slot of a batch is accepted; table[slot][try - 1] = (classes, nonbg)."""
    has_fg, out = 0, []
    for slot in range(batch_size):
        t, change, _, _ = slot_tries(table[slot], slot, has_fg, batch_size, n_classes, fg_batch_fraction, force_all_fg,
                                     max_tries)
        assert t is not None, "table row shorter than max_tries"
        has_fg += change
        out.append(t)
    return out
