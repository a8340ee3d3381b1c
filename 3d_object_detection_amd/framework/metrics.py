"""framework.metrics.Metric (reference metrics.py:5-52): precision / recall of sigmoid(cls) at 0.1 / 0.3 / 0.5 / 0.7 over the anchors
with label != -1.  The tp / tn / fp / fn counts are those of pp_target_loss (assign.hip), integers summed on the device."""
import numpy as np
import torch

from ..engine import engine_for, engine_for_anchors

THRESHOLDS = [0.1, 0.3, 0.5, 0.7]


class Metric:
    def __init__(self, config=None):
        """Metric() as the reference builds it (metrics.py:6): the engine is then the live one whose anchor count matches the
        logits given to update(); Metric(config) names it through the config dict instead."""
        self._thresholds = list(THRESHOLDS)
        self._config = config
        num = len(self._thresholds)
        self.rec_count = torch.zeros(num)
        self.rec_total = torch.zeros(num)
        self.prec_count = torch.zeros(num)
        self.prec_total = torch.zeros(num)

    def update_counts(self, counts):
        """counts [4 thresholds, (tp, tn, fp, fn)] of one update (a batch); also accepts terms f64[B, PP_LOSS_TERMS]."""
        c = np.asarray(counts.cpu() if isinstance(counts, torch.Tensor) else counts, dtype=np.float64)
        if c.ndim == 2 and c.shape[1] > 16:
            c = c[:, 5:21].sum(0)
        c = c.reshape(len(self._thresholds), 4)
        for i in range(len(self._thresholds)):
            tp, tn, fp, fn = c[i]
            if tp + fn > 0:
                self.rec_count[i] += tp + fn
                self.rec_total[i] += tp
            if tp + fp > 0:
                self.prec_count[i] += tp + fp
                self.prec_total[i] += tp

    def update(self, labels, preds, weights=None):
        """The reference's signature: labels [B,A] (numpy or torch), preds = cls logits [B,A(,1)]."""
        if weights is not None:
            raise ValueError("Metric.update: only the reference's default weights (label != -1) are supported")
        lab = labels if isinstance(labels, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(labels))
        B = int(lab.shape[0])
        if self._config is not None:
            eng = engine_for(self._config)
        else:
            dev = preds.device if isinstance(preds, torch.Tensor) and preds.is_cuda else torch.device("cuda", torch.cuda.current_device())
            eng = engine_for_anchors(lab.numel() // max(B, 1), dev)
        dev = eng.device
        lab = lab.to(dev, torch.int32).reshape(B, -1).contiguous()
        cls = preds.to(dev, torch.float32).reshape(B, -1).contiguous()
        # counts only: pp_target_loss without the regression inputs
        terms = [eng.target_loss(cls[i:i + eng.max_batch], None, None, lab[i:i + eng.max_batch], None, None)
                 for i in range(0, B, eng.max_batch)]
        self.update_counts(torch.cat(terms))

    def __str__(self):
        str = ""
        prec, rec = self.value
        for i, t in enumerate(self._thresholds):
            str += "@%.2f prec:%.5f, rec:%.5f  " % (t, prec[i], rec[i])
        return str

    @property
    def value(self):
        prec_count = torch.clamp(self.prec_count, min=1.0)
        rec_count = torch.clamp(self.rec_count, min=1.0)
        return (self.prec_total / prec_count).cpu(), (self.rec_total / rec_count).cpu()

    def clear(self):
        self.rec_count.zero_()
        self.prec_count.zero_()
        self.prec_total.zero_()
        self.rec_total.zero_()
