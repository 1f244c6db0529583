#!/bin/bash
# A/B of the train step's time, one GPU, one call: the cross-entropy step of another checkout (the parent commit, built) and of
# this one, alternating, three times; then the step under each loss of mpunet/evaluate/loss_functions.py. tools/time_losses.py
# does one measurement (graph replay, 10 warm-up + 50 timed steps between events, 3 repeats). Every step runs under its own time
# limit and the chain stops at the first failure.
#   tools/time_losses.sh PARENT_CHECKOUT OUT.jsonl
set -u
cd "$(dirname "$0")/.."
PARENT=${1:?usage: tools/time_losses.sh PARENT_CHECKOUT OUT.jsonl}
OUT=${2:?usage: tools/time_losses.sh PARENT_CHECKOUT OUT.jsonl}
T="timeout -k 10 240 python tools/time_losses.py"
: > "$OUT"
$T --root "$PARENT" --tag parent_ce >> "$OUT" && $T --tag ce >> "$OUT" &&
$T --root "$PARENT" --tag parent_ce >> "$OUT" && $T --tag ce >> "$OUT" &&
$T --root "$PARENT" --tag parent_ce >> "$OUT" && $T --tag ce >> "$OUT" &&
$T --tag dice --loss SparseDiceLoss --loss-kwargs '{"smooth": 1}' >> "$OUT" &&
$T --tag jaccard --loss SparseJaccardDistanceLoss --loss-kwargs '{"smooth": 1}' >> "$OUT" &&
$T --tag gdl_square --loss SparseGeneralizedDiceLoss --loss-kwargs '{"type_weight": "Square"}' >> "$OUT" &&
$T --tag focal --loss SparseFocalLoss --loss-kwargs '{"gamma": 2, "class_weights": [0.2, 1, 1]}' >> "$OUT" &&
$T --tag explog --loss SparseExponentialLogarithmicLoss >> "$OUT" &&
$T --root "$PARENT" --tag parent_ce >> "$OUT" && $T --tag ce >> "$OUT"
rc=$?
cat "$OUT"
exit $rc
