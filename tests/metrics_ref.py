"""
TEST INFRASTRUCTURE ONLY. NumPy (f64) restatement of the training metrics `fit.metrics` can name, as Keras computes them for
`compile(metrics=[...])` under TF 2.3: tf.keras.metrics.sparse_categorical_accuracy and the five sparse_* functions of the
reference's mpunet/evaluate/metrics.py, each wrapped in a Keras `Mean` (per batch total += sum(values), count += size(values);
result total / count, 0 where count == 0). Written from the TF documentation of tf.argmax (first maximum), tf.math.confusion_matrix
(without num_classes: 1 + the largest value in labels or predictions) and tf.linalg.diag_part -- the renamed forms of the TF-1 names
the three sparse_mean_fg_* functions call. Metrics are unweighted. The TensorFlow binary is absent (as for tests/loss_ref.py): the
restatement is anchored on the hand-computed known answers of tests/test_train_metrics_host.py.
"""
import numpy as np

NAMES = ("sparse_categorical_accuracy", "sparse_fg_recall", "sparse_fg_precision", "sparse_mean_fg_precision",
         "sparse_mean_fg_recall", "sparse_mean_fg_f1")


def argmax_first(scores):
    """tf.argmax over the last axis: the first maximum."""
    return np.argmax(np.asarray(scores), axis=-1)


def confusion_matrix(y, pred):
    """tf.math.confusion_matrix(labels, predictions) with num_classes left out: rows = labels, columns = predictions."""
    k = int(max(y.max(), pred.max())) + 1
    cm = np.zeros((k, k), np.int64)
    np.add.at(cm, (y, pred), 1)
    return cm


def batch_values(y, pred):
    """One batch: {name: (sum of the metric function's values, their number)} for labels y and predicted classes pred (any
    shape, flattened). 0 / 0 is NaN and is kept."""
    y = np.asarray(y).reshape(-1).astype(np.int64)
    pred = np.asarray(pred).reshape(-1).astype(np.int64)
    out = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        hit = y == pred
        out["sparse_categorical_accuracy"] = (float(hit.sum()), float(y.size))           # one 0/1 value per pixel
        # mean of the hits over the pixels whose LABEL (recall) / PREDICTION (precision) is not background
        fg_y, fg_p = y != 0, pred != 0
        out["sparse_fg_recall"] = (np.float64(hit[fg_y].sum()) / np.float64(fg_y.sum()), 1.0)
        out["sparse_fg_precision"] = (np.float64(hit[fg_p].sum()) / np.float64(fg_p.sum()), 1.0)
        cm = confusion_matrix(y, pred).astype(np.float64)
        tp = np.diag(cm)
        precisions = tp / cm.sum(axis=0)              # column sums: how often each class was predicted
        recalls = tp / cm.sum(axis=1)                 # row sums: how often each class was the label
        f1s = (2 * precisions * recalls) / (precisions + recalls)
        mean = lambda v: np.float64(np.sum(v)) / np.float64(v.size)     # reduce_mean; of nothing: 0 / 0
        out["sparse_mean_fg_precision"] = (mean(precisions[1:]), 1.0)
        out["sparse_mean_fg_recall"] = (mean(recalls[1:]), 1.0)
        out["sparse_mean_fg_f1"] = (mean(f1s[1:]), 1.0)
    return {k: (float(t), float(c)) for k, (t, c) in out.items()}


def batch_metrics(y, pred):
    """{name: the value Keras reports for this batch alone}."""
    return {k: (t / c if c else 0.0) for k, (t, c) in batch_values(y, pred).items()}


class Mean:
    """The six Keras Means over a sequence of batches."""

    def __init__(self):
        self.total = {k: 0.0 for k in NAMES}
        self.count = {k: 0.0 for k in NAMES}

    def update(self, y, pred):
        for k, (t, c) in batch_values(y, pred).items():
            self.total[k] += t
            self.count[k] += c
        return self

    def update_scores(self, y, scores):
        return self.update(y, argmax_first(scores))

    def result(self):
        return {k: (self.total[k] / self.count[k] if self.count[k] else 0.0) for k in NAMES}
