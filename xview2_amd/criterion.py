"""Loss composition on the fused HIP loss kernels: drop-in for the reference's model/loss.py ``Loss``.

``--loss_str`` is a '+'-separated sum of dice, focal, ce, ohem (model/loss.py:68-83).  dice/focal are the
monai 0.4.0 losses with the constructor arguments of model/loss.py:11-13; ``mse`` / ``coral`` (model/loss.py:54-65,92-94) have their own kernels; ``ohem`` is numerically the mean
cross-entropy (the reference slices the (values, indices) tuple of ``sort`` at model/loss.py:45, so no
negative is ever dropped).  All terms of one call share a single softmax pass; for ``--type post`` the
building mask of model/loss.py:86-90 is applied inside the kernels (no compaction, order-independent sums).

``ohem_hard`` is the hard-negative mining that ``ohem`` is named after, i.e. the reference's Ohem with the tuple slip
repaired: per image every positive pixel (label > 0) and the k = min(Cn, max(Cn // 4, 5, 2 Cp)) negatives with the
largest cross-entropy, summed over the batch and divided by the number of kept pixels (``ops.OhemFn``).  Negatives tied
with the k-th largest loss share the remaining places: each gets the gradient weight r / c_eq (the mean over every valid
choice of the tied subset), which differs from autograd through ``sort`` only on exact ties.  Under ``--type post`` the
reference hands Ohem one row per building pixel, each keeps its single entry (k >= 1), so ``ohem_hard`` is mean CE over
building pixels there and is routed to the CE bit.

``lovasz`` is the Lovasz-softmax loss (Berman et al., CVPR 2018, Algorithm 1; ``ops.LovaszFn``, csrc/lovasz.hip) with
classes "present" over the whole batch: the convex extension of the Jaccard loss, which the xView2 F1 scores follow.
``--type pre`` averages over the building class alone (dice drops the background for two channels the same way);
``--type post`` over the four damage classes on building pixels, label 0 being in no class's set.  It is not in the
reference's list; it is usually joined with a per-pixel term (``lovasz+ce``, ``focal+lovasz``).

``wce`` is cross-entropy with a per-pixel weight (``ops.WceFn``, csrc/wce.hip): sum w l / sum w with w = cw[class] + b.
``--class_weights`` gives cw (none: all ones; with b = 0 the term is ``torch.nn.functional.cross_entropy(weight=cw)``);
``--border_weight W0`` adds the U-Net paper's border map b = W0 exp(-(d1 + d2)^2 / (2 S^2)) (Ronneberger et al. 2015) with
d1 / d2 the distances from a background pixel to the two nearest labelled buildings within ``--border_radius`` pixels and
S = ``--border_sigma``: the narrow gaps between neighbouring buildings become expensive to get wrong.  ``--type pre`` only;
``compute_loss`` computes the distance maps once per batch, on the full-resolution labels, and every head reads them.
"""
import math

import torch
from torch import nn

from . import ops

_TERM_BITS = {"dice": ops.LOSS_DICE, "focal": ops.LOSS_FOCAL, "ce": ops.LOSS_CE, "ohem": ops.LOSS_CE}
BORDER_RADIUS_MAX = 32


def parse_class_weights(value, n_class):
    """--class_weights: None (all ones), a 'w0,w1[,w2,w3]' string or a sequence -> n_class finite floats >= 0, not all zero"""
    if value is None:
        return [1.0] * n_class
    try:
        w = [float(v) for v in (value.split(",") if isinstance(value, str) else value)]
    except (TypeError, ValueError):
        raise ValueError("--class_weights %r: comma-separated numbers expected" % (value,))
    if len(w) != n_class:
        raise ValueError("--class_weights %r: %d weights for %d classes (2 for --type pre, 4 for --type post)"
                         % (value, len(w), n_class))
    if not all(math.isfinite(v) and v >= 0.0 for v in w):
        raise ValueError("--class_weights %r: every weight must be finite and >= 0" % (value,))
    if not any(v > 0.0 for v in w):
        raise ValueError("--class_weights %r: at least one weight must be > 0" % (value,))
    return w


class Loss(nn.Module):
    def __init__(self, args):
        super().__init__()
        self.loss_str = args.loss_str
        self.post = args.type == "post"
        self.names = self.loss_str.split("+")
        for n in self.names:
            if n not in ("dice", "focal", "ce", "ohem", "ohem_hard", "lovasz", "wce", "mse", "coral"):
                raise KeyError(n)
        # The reference special-cases loss_str == "mse" (float targets, model/loss.py:92-94) and builds the 3-logit coral head
        # only for loss_str == "coral" (model/unet.py:21-26): combined with other terms both fail in the reference's FIRST
        # forward with a RuntimeError (nn.MSELoss on [M, 4] logits against [M] long labels: "The size of tensor a (4) must match
        # the size of tensor b (M)"; CORAL's [M, 4] logits against its [M, 3] levels: "... tensor a (4) ... tensor b (3) ...").
        # Same here: construction succeeds, the first forward raises RuntimeError.
        self.unsupported_combo = ("mse" in self.names or "coral" in self.names) and len(self.names) > 1
        # the weights of "wce"; golden argument objects without the attributes get the defaults of main.py
        self.border_weight = float(getattr(args, "border_weight", 0.0))
        self.border_sigma = float(getattr(args, "border_sigma", 5.0))
        self.border_radius = int(getattr(args, "border_radius", 0))
        cw = parse_class_weights(getattr(args, "class_weights", None), 4 if self.post else 2)
        if not (math.isfinite(self.border_weight) and self.border_weight >= 0.0):
            raise ValueError("--border_weight %r: must be finite and >= 0" % (self.border_weight,))
        if not (math.isfinite(self.border_sigma) and self.border_sigma > 0.0):
            raise ValueError("--border_sigma %r: must be finite and > 0" % (self.border_sigma,))
        if not 0 <= self.border_radius <= BORDER_RADIUS_MAX:
            raise ValueError("--border_radius %r: must be in 0..%d (0: min(%d, ceil(3 sigma)))"
                             % (self.border_radius, BORDER_RADIUS_MAX, BORDER_RADIUS_MAX))
        if self.border_weight > 0.0 and self.post:
            raise ValueError("--border_weight %g with --type post: the border map is defined for --type pre only"
                             % self.border_weight)
        if self.border_radius == 0:
            self.border_radius = min(BORDER_RADIUS_MAX, max(1, math.ceil(3.0 * self.border_sigma)))
        self.wants_border = "wce" in self.names and self.border_weight > 0.0
        self.class_weights = cw
        self._class_w = None      # the weights as a device tensor, made on the first wce call (no buffer: state_dict keeps its keys)

    def class_w(self, device):
        if self._class_w is None or self._class_w.device != device:
            self._class_w = torch.tensor(self.class_weights, dtype=torch.float32, device=device)
        return self._class_w

    def border_maps(self, y_true):
        """the distance maps of one batch of FULL-RESOLUTION labels for the wce term, or None when it has no border part"""
        if not self.wants_border:
            return None
        return ops.border_distances(y_true, self.border_radius)

    def forward(self, y_pred, y_true, label_stride=1, border=None):
        """y_pred NCHW logits; y_true [N, H*label_stride, W*label_stride] uint8/long labels; border: what
        ``border_maps(y_true)`` returned for these labels (None: computed here when the wce term wants it)."""
        if self.unsupported_combo:
            bad = "mse" if "mse" in self.names else "coral"
            raise RuntimeError("--loss_str %s: the size of tensor a (%d) must match the size of tensor b (%s) at non-singleton "
                               "dimension 1 (%s does not compose with other loss terms: model/loss.py:92-99 fails the same way)"
                               % (self.loss_str, y_pred.shape[1], "3" if bad == "coral" else "M", bad))
        if self.names[0] in ("mse", "coral"):
            bits = ops.LOSS_MSE if self.names[0] == "mse" else ops.LOSS_CORAL
            return ops.LossFn.apply(y_pred, y_true, bits, self.post, label_stride)
        # the reference sums the terms one by one; duplicated names count twice
        total = None
        counts = {}
        hard = lovasz = wce = 0
        for n in self.names:
            if n == "ohem_hard" and not self.post:
                hard += 1
                continue
            if n == "lovasz":
                lovasz += 1
                continue
            if n == "wce":
                wce += 1
                continue
            b = ops.LOSS_CE if n == "ohem_hard" else _TERM_BITS[n]
            counts[b] = counts.get(b, 0) + 1
        while counts:
            bits = 0
            for b in list(counts):
                bits |= b
                counts[b] -= 1
                if counts[b] == 0:
                    del counts[b]
            part = ops.LossFn.apply(y_pred, y_true, bits, self.post, label_stride)
            total = part if total is None else total + part
        for _ in range(hard):
            part = ops.OhemFn.apply(y_pred, y_true, label_stride)
            total = part if total is None else total + part
        for _ in range(lovasz):
            part = ops.LovaszFn.apply(y_pred, y_true, label_stride, self.post)
            total = part if total is None else total + part
        if wce:
            if border is None:
                border = self.border_maps(y_true)
            d1, d2 = (None, None) if border is None else border
            cw = self.class_w(y_pred.device)
            for _ in range(wce):
                part = ops.WceFn.apply(y_pred, y_true, cw, label_stride, self.post, d1, d2, self.border_weight,
                                       self.border_sigma)
                total = part if total is None else total + part
        return total


def compute_loss(loss_fn, preds, label, deep_supervision):
    """model/plt.py:69-77: L(out) + 1/2 L(out_dec4, lbl[::2, ::2]) + 1/4 L(out_dec3, lbl[::4, ::4]), times
    1/(2 - 2^-3); the nearest-neighbour label down-sampling is index arithmetic inside the loss kernel."""
    if not deep_supervision:
        return loss_fn(preds, label)
    # the wce term's distance maps: once per batch, before the heads, which all read them (None otherwise: nothing is launched)
    kw = {"border": loss_fn.border_maps(label)} if getattr(loss_fn, "wants_border", False) else {}
    loss = loss_fn(preds[0], label, **kw)
    for i, pred in enumerate(preds[1:]):
        stride = label.shape[-1] // pred.shape[-1]
        loss = loss + 0.5 ** (i + 1) * loss_fn(pred, label, label_stride=stride, **kw)
    c_norm = 1 / (2 - 2 ** (-len(preds)))
    return c_norm * loss
