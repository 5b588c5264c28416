"""Inference post-processing: model outputs -> the ranked `pred_relevant_windows` rows of the
reference's submission format (eval.py:63-92, utils/post_processing.py:22-47).

The per-query arithmetic (foreground softmax score, centre/width -> start/end, x duration) runs as
one kernel (`mesm_windows`); ranking and the reference's decimal formatting
(float(f"{e:.4f}"), then clamp / round-to-clip-length in float32 with half-to-even rounding) are
host work on N x Q x 3 numbers in `predict_windows`, done in numpy so that the rows are identical to the
reference's, digit for digit.  `predict_windows` is the referee of `device_rows`, which does all of it
in one kernel (`mesm_windows_rows`) and is what `compute_mr_results` uses.
"""
import numpy as np
import torch

from ._lib import check, lib, ptr, require_gpu, stream_ptr
from .criterion import loss_pack


def raw_windows(pred_logits, pred_spans, duration):
    """(N, Q, 2) logits, (N, Q, 2) spans (centre, width; normalised), (N,) durations -> (N, Q, 3)
    float32 [start, end, foreground score] on the device."""
    require_gpu(pred_logits, pred_spans, duration)
    lg = pred_logits.detach().float().contiguous()
    sp = pred_spans.detach().float().contiguous()
    du = duration.detach().float().contiguous()
    N, Q, _ = lg.shape
    out = torch.empty(N, Q, 3, device=lg.device, dtype=torch.float32)
    check(lib().mesm_windows(ptr(lg), ptr(sp), ptr(du), ptr(out), N, Q, stream_ptr()), "mesm_windows")
    return out


def device_rows(pred_logits, pred_spans, duration, clip_len=2, max_ts_val=150, min_ts_val=0, sort_results=True):
    """predict_windows on the device: (N, Q, 3) float64 rows [start, end, score], ranked, rounded, clamped and snapped
    exactly like predict_windows (its .tolist() is predict_windows' result).  One wave per query: Q <= 64."""
    require_gpu(pred_logits, pred_spans, duration)
    lg = pred_logits.detach().float().contiguous()
    sp = pred_spans.detach().float().contiguous()
    du = duration.detach().float().contiguous()
    N, Q, _ = lg.shape
    out = torch.empty(N, Q, 3, device=lg.device, dtype=torch.float64)
    check(lib().mesm_windows_rows(ptr(lg), ptr(sp), ptr(du), ptr(out), N, Q, float(np.float32(clip_len)),
                                  float(np.float32(min_ts_val)), float(np.float32(max_ts_val)), int(bool(sort_results)),
                                  stream_ptr()), "mesm_windows_rows")
    return out


def round4_emulated(a):
    """the kernel's float(f"{x:.4f}") for float32 `a`: rint(double(x) * 1e4) / 1e4 in fp64 (exact product, half-to-even
    rounding of the exact decimal value, correctly rounded division)"""
    return np.rint(np.asarray(a, dtype=np.float32).astype(np.float64) * 1e4) / 1e4


def _round4(a):
    """float(f"{e:.4f}") element-wise: decimal rounding of the float32 value widened to double."""
    flat = a.astype(np.float64).ravel()
    return np.array([float("%.4f" % e) for e in flat], dtype=np.float64).reshape(a.shape)


def predict_windows(pred_logits, pred_spans, duration, clip_len=2, max_ts_val=150, min_ts_val=0,
                    sort_results=True):
    """-> list (per query) of Q rows [start, end, score] exactly as eval.py + PostProcessorDETR emit."""
    raw = raw_windows(pred_logits, pred_spans, duration).cpu().numpy()  # float32
    out = []
    for rows in raw:
        if sort_results:
            order = sorted(range(rows.shape[0]), key=lambda i: float(rows[i, 2]), reverse=True)  # stable
            rows = rows[order]
        r4 = _round4(rows)
        w = np.clip(r4[:, :2].astype(np.float32), np.float32(min_ts_val), np.float32(max_ts_val))
        if clip_len != -1:
            w = np.round(w / np.float32(clip_len)) * np.float32(clip_len)  # half to even, float32 like torch.round
        sc = _round4(r4[:, 2].astype(np.float32))
        out.append([[float(w[i, 0]), float(w[i, 1]), float(sc[i])] for i in range(rows.shape[0])])
    return out


# ----------------------------------------------------------------------------- submission rows + NMS
def saliency_rows(saliency_scores, video_mask):
    """eval.py:66-71: the per-clip scores in fp16 (`.half()`), one list per query cut at its video length."""
    s16 = saliency_scores.detach().to(torch.float16)
    lens = video_mask.sum(1).cpu().tolist()
    s16 = s16.cpu()
    return [s16[j, :int(lens[j])].tolist() for j in range(len(lens))]


def compute_temporal_iou(pred, gt):
    """utils/temporal_nms.py:6-22: intersection over the HULL of the two windows (the reference's own
    "not the correct union")."""
    inter = max(0, min(pred[1], gt[1]) - max(pred[0], gt[0]))
    union = max(pred[1], gt[1]) - min(pred[0], gt[0])
    return 0 if union == 0 else 1.0 * inter / union


def temporal_nms(predictions, nms_thd, max_after_nms=100):
    """utils/temporal_nms.py:25-74: greedy NMS over [start, end, score] rows, best score first; a row is
    dropped when its IoU with a kept row exceeds nms_thd; at most max_after_nms rows survive."""
    if len(predictions) == 1:
        return predictions
    rest = sorted(predictions, key=lambda x: x[2], reverse=True)
    kept = []
    while len(rest) > 1 and len(kept) < max_after_nms:
        head = rest[0]
        rest = [head] + [r for r in rest[1:] if not compute_temporal_iou(head[:2], r[:2]) > nms_thd]
        kept.append(rest.pop(0))
    if len(kept) < max_after_nms and len(rest) >= 1:
        kept.append(rest.pop(0))
    return [[st, ed, s] for st, ed, s in kept]


def post_processing_mr_nms(mr_res, nms_thd, max_before_nms, max_after_nms):
    """eval.py:476-485."""
    out = []
    for e in mr_res:
        e["pred_relevant_windows"] = temporal_nms(e["pred_relevant_windows"][:max_before_nms], nms_thd=nms_thd,
                                                  max_after_nms=max_after_nms)
        out.append(e)
    return out


class _BatchFetch:
    """the host half of one evaluation batch in ONE device-to-host transfer: the submission rows (float64), the loss
    vector and the per-query video lengths, then the fp16 saliency scores, packed byte-wise into a pinned buffer"""

    def __init__(self):
        self.pinned = None

    def __call__(self, parts):
        flat = torch.cat([t.contiguous().view(-1).view(torch.uint8) for t in parts])
        n = flat.numel()
        if self.pinned is None or self.pinned.numel() < n:
            self.pinned = torch.empty(max(2 * n, 1 << 16), dtype=torch.uint8, pin_memory=True)
        self.pinned[:n].copy_(flat, non_blocking=True)
        torch.cuda.current_stream(flat.device).synchronize()
        raw = self.pinned.numpy()[:n]
        res, off = [], 0
        for t in parts:
            nb = t.numel() * t.element_size()
            res.append(raw[off:off + nb].view(str(t.dtype).replace("torch.", "")).reshape(tuple(t.shape)).copy())
            off += nb
        return res


def _loss_vector(loss_dict, loss, device):
    """(names, 1-D float tensor on `device` whose entries are the eager float() values of loss_dict[name] in order, then
    `loss`); entries may be tensors or plain numbers"""
    names = list(loss_dict)
    vals = list(loss_dict.values())
    pack = loss_pack(loss_dict)
    if pack is not None and torch.is_tensor(loss) and pack.vec.dtype == loss.dtype and loss.device == pack.vec.device:
        idx = torch.tensor([int(v._i) for v in vals], device=pack.vec.device)
        return names, torch.cat([pack.vec.detach()[idx], loss.detach().reshape(1)]).to(device)
    f64 = lambda v: (v.detach() if torch.is_tensor(v) else torch.as_tensor(float(v), dtype=torch.float64)).to(device=device, dtype=torch.float64).reshape(())
    return names, torch.stack([f64(v) for v in vals] + [f64(loss)])


@torch.no_grad()
def compute_mr_results(model, eval_loader, opt, criterion=None, prepare=None):
    """eval.py:52-117: model.eval(), one forward per batch with is_training=False, submission rows
    (`pred_relevant_windows` ranked + clamped + rounded to clip_len multiples, `pred_saliency_scores`), and the
    weighted loss meters when a criterion is given.  `prepare(batch)` moves a host batch to the device
    (mesm_amd.batching.prepare_batch_input); None = the batches are already there.  Per batch: the rows on the device
    (device_rows), then ONE transfer of rows, saliency and losses (the reference formats every number in Python and
    synchronises once per loss entry)."""
    model.eval()
    if criterion is not None:
        criterion.eval()
    sums, counts = {}, {}
    mr_res = []
    fetch = _BatchFetch()
    for batch in eval_loader:
        if prepare is not None:
            batch = prepare(batch)
        outputs = model(**batch, dataset_name=opt.dataset_name, is_training=False)
        rows = device_rows(outputs["pred_logits"], outputs["pred_spans"], batch["duration"],
                           clip_len=opt.clip_len, max_ts_val=opt.max_ts_val,
                           sort_results=getattr(opt, "sort_results", True))
        vm = batch["video_mask"]
        lens = vm.sum(1, dtype=torch.int64) if vm.is_cuda else vm.sum(1).to(torch.int64).to(rows.device)
        parts = [rows, lens]
        names = None
        if criterion is not None:
            loss_dict, loss = criterion(outputs, batch, is_training=False)
            names, lv = _loss_vector(dict(loss_dict), loss, rows.device)
            parts.append(lv)
        parts.append(outputs["saliency_scores"].detach().to(torch.float16))  # eval.py:66 (.half())
        got = fetch(parts)
        rows_h, lens_h, s16 = got[0].tolist(), got[1].tolist(), got[-1]
        for idx in range(len(rows_h)):
            mr_res.append(dict(qid=batch["qid"][idx], query=batch["sentence"][idx], vid=batch["video_id"][idx],
                               pred_relevant_windows=rows_h[idx], pred_saliency_scores=s16[idx, :lens_h[idx]].tolist()))
        if criterion is not None:
            vals = got[2].tolist()
            for k, v in zip(names + ["loss_overall"], vals):
                w = criterion.weight_dict[k] if k in criterion.weight_dict else 1.0
                sums[k] = sums.get(k, 0.0) + float(v) * w
                counts[k] = counts.get(k, 0) + 1
    return mr_res, {k: sums[k] / counts[k] for k in sums}
