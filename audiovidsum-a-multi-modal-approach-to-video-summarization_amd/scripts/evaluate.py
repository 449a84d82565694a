"""Counterpart of the reference's scripts/evaluate.py:6-42: score every video of a dataset with the model (one
video per call, B = 1, on the MI355X), then the per-video mean-threshold F1 and rank correlations, averaged.
Same signature and return keys as the reference; the metric arithmetic lives in evaluation.metrics.
evaluate_batch is the same evaluation as one ragged batch: one score_rows call, the metrics on the device, one download."""
import torch

from ..evaluation.metrics import summarize_scores, summarize_scores_device
from ..ragged import exclusive_offsets


def predict_dataset(model, dataset):
    """[(pred [S], target [S])] as numpy arrays, model in eval mode, no autograd."""
    model.eval()
    pairs = []
    with torch.no_grad():
        for features, scores in dataset:
            inputs = [features[k].unsqueeze(0).cuda() for k in ("visual", "audio")]
            pairs.append((model(*inputs).cpu().squeeze().numpy(), scores.numpy()))
    return pairs


def evaluate(model, dataset):
    return summarize_scores(predict_dataset(model, dataset))


def evaluate_batch(model, dataset):
    """evaluate() for the whole dataset at once: the videos' features are uploaded once into concatenated device
    matrices, scored by one model.score_rows call (each video its own recurrence, attn_batch = 1: bit for bit the
    per-video B = 1 scores), and the metrics come from summarize_scores_device.  Same return keys as evaluate.  The targets keep their dtype,
    float32 or float64; any other is refused, since converting a target moves its ties and its mean threshold."""
    model.eval()
    items, lengths = [], []
    for features, scores in dataset:
        scores = torch.as_tensor(scores)
        if scores.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"evaluate_batch: targets must be float32 or float64, got {scores.dtype}")
        if items and scores.dtype != items[0][2].dtype:
            raise ValueError(f"evaluate_batch: the targets mix {items[0][2].dtype} and {scores.dtype}")
        visual, audio, scores = features["visual"], features["audio"], scores.reshape(-1)
        if visual.dim() != 2 or audio.dim() != 2 or not visual.shape[0] == audio.shape[0] == scores.shape[0]:
            raise ValueError(f"evaluate_batch: video {len(items)} has visual {tuple(visual.shape)}, audio "
                             f"{tuple(audio.shape)} and {scores.shape[0]} target scores")
        items.append((visual, audio, scores))
        lengths.append(visual.shape[0])
    if not items:
        raise ValueError("evaluate_batch: empty dataset")
    offsets = exclusive_offsets(lengths)
    dev = torch.device("cuda", torch.cuda.current_device())
    from .. import ops
    tables = ops.EvalTables(offsets, dev)
    # every video goes straight into its rows of the device matrices: no concatenated copy on the host
    visual = torch.empty((tables.rows, items[0][0].shape[1]), dtype=torch.float32, device=dev)
    audio = torch.empty((tables.rows, items[0][1].shape[1]), dtype=torch.float32, device=dev)
    target = torch.empty(tables.rows, dtype=items[0][2].dtype, device=dev)
    for (v, a, s), r0, r1 in zip(items, offsets[:-1], offsets[1:]):
        visual[r0:r1].copy_(v)
        audio[r0:r1].copy_(a)
        target[r0:r1].copy_(s)
    with torch.no_grad():
        pred = model.score_rows(visual, audio, tables.offsets_t, attn_batch=1)
        return summarize_scores_device(pred, target, tables)
