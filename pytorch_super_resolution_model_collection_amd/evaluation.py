"""The evaluation bookkeeping of _Trainer.test(), test_single(path) and main.report(): one table of metrics (METRICS), one
accumulator (Scores) that serves the net's output and the loader's bicubic picture alike, and the report line formatted
from the same table.  A new metric is one new row.  DESIGN.md section 36 has the rules.

A row (o: the call's Options):
  key, label          results go to <trainer>.test_<key>[dataset]; label: the %-format of the stored value in the report
  per_side            True: also test_bicubic_<key>, printed in each side's group; False: net only, a group of its own
  enabled(o)          whether the call produces it at all; a row that is off leaves its attributes untouched
  needs_target        True: only for a picture whose target has the same shape
  fits(pic, o)        whether this picture qualifies; one that does not is left out silently
  value(pic, tgt, o)  the picture's value as a DEVICE tensor: nothing here may read a device value back
  host(vals, o)       after the dataset: the per-picture host values, in loader order, of the device values collected
  mean(host, o)       the stored number of a dataset from its (non-empty) per-picture host values"""
import collections

import torch

from . import ops, utils

Metric = collections.namedtuple("Metric", "key label per_side enabled needs_target fits value host mean")


class Options(object):
    """What the rows read of a call: the trainer (its lpips_net() and niqe_params(); None: that row is off) and the
    eval_domain / eval_shave pair (None: not given; the row is on when either is, and the other is then 'float' / 0)."""

    def __init__(self, trainer, eval_domain=None, eval_shave=None):
        self.trainer, self.want_eval = trainer, eval_domain is not None or eval_shave is not None
        self.eval_domain = "float" if eval_domain is None else eval_domain
        self.eval_shave = 0 if eval_shave is None else int(eval_shave)


def _side(pic):
    return min(int(pic.shape[-2]), int(pic.shape[-1]))


def _floats(vals, o):
    return [float(v) for v in torch.stack(vals).cpu()]      # one stacked device-to-host copy


def _mean(host, o):
    return sum(host) / len(host)


def _planes(img):      # [C,H,W] of [1,C,H,W] / [C,H,W] float, or of [H,W,3] / [H,W] uint8 as the picture tail writes it
    if img.dtype == torch.uint8:
        return img.unsqueeze(0) if img.dim() == 2 else img.permute(2, 0, 1)
    return (img[0] if img.dim() == 4 else img).float()


def _niqe_fits(img, o):      # two 96 x 96 blocks at least after the shave, one or three channels
    c, h, w = _planes(img).shape
    nh, nw = ops.niqe_blocks(h, w, o.eval_shave)
    return c in (1, 3) and nh * nw >= 2


def _niqe_scores(feats, o):      # the 36 x 36 finish (host arithmetic); fewer than two NaN-free blocks: left out
    host = []
    for f in feats:
        try:
            host.append(ops.niqe_finish(f, *o.trainer.niqe_params()))
        except ValueError:
            pass
    return host


METRICS = (
    Metric("psnr", "PSNR %.4f", True, lambda o: True, True, lambda pic, o: True,
           lambda pic, tgt, o: utils.PSNR(pic, tgt), _floats, _mean),
    Metric("ssim", "SSIM %.4f", True, lambda o: True, True, lambda pic, o: _side(pic) >= 11,      # the 11 x 11 window
           lambda pic, tgt, o: utils.SSIM(pic, tgt), _floats, _mean),
    Metric("lpips", "LPIPS %.4f", True, lambda o: o.trainer.lpips_net() is not None, True,
           lambda pic, o: _side(pic) >= 16,                                                       # the five taps need 16
           torch.no_grad()(lambda pic, tgt, o: ops.lpips(pic.float(), tgt.float(), o.trainer.lpips_net(), normalize=True,
                                                         reduce=True)), _floats, _mean),
    # of the 8-bit picture, eval_shave pixels off each side; the features stay on the device, the finish is `host`
    Metric("niqe", "NIQE %.4f", True, lambda o: o.trainer.niqe_params() is not None, False, _niqe_fits,
           lambda pic, tgt, o: ops.niqe_features(_planes(pic), o.eval_shave), _niqe_scores, _mean),
    # --eval_domain / --eval_shave: ops.ssim's fused (ssim, psnr) in that domain with that border left out
    Metric("eval", "%(domain)s shave %(shave)d: PSNR %(psnr).4f SSIM %(ssim).4f", False, lambda o: o.want_eval, True,
           lambda pic, o: _side(pic) - 2 * o.eval_shave >= 11,
           lambda pic, tgt, o: torch.stack(ops.ssim(pic.float(), tgt.float(), o.eval_shave, o.eval_domain)[:2]),
           lambda vals, o: [(float(s), float(p)) for s, p in torch.stack(vals).double().cpu()],
           lambda host, o: dict(domain=o.eval_domain, shave=o.eval_shave, psnr=_mean([p for _, p in host], o),
                                ssim=_mean([s for s, _ in host], o))),
)
RETURNED = "psnr"      # test() returns this row's per-picture values of the net's side


class Scores(object):
    """The enabled rows of one side over a call: creates owner.test_<key> = {} (bicubic: owner.test_bicubic_<key>, per_side
    rows only), collects device values picture by picture (add) and stores a dataset's numbers (finish).  An attribute
    of a row that is off is neither created nor touched; a dataset gets a key only where a picture counted."""

    def __init__(self, owner, opts, bicubic=False, metrics=METRICS):
        rows = [m for m in metrics if m.enabled(opts) and (m.per_side or not bicubic)]
        self.rows, self.opts = sorted(rows, key=lambda m: m.needs_target), opts      # (stable: rows without a target first)
        self.stored, self.vals = {m.key: {} for m in rows}, {m.key: [] for m in rows}
        for key, into in self.stored.items():
            setattr(owner, ("test_bicubic_" if bicubic else "test_") + key, into)

    def add(self, pic, tgt=None):
        """One picture (on the device) and its target; tgt None or of another shape: only the rows that need none."""
        paired = tgt is not None and pic.shape == tgt.shape
        for m in self.rows:
            if (paired or not m.needs_target) and m.fits(pic, self.opts):
                self.vals[m.key].append(m.value(pic, tgt, self.opts))

    def finish(self, name):
        """Stores the numbers of dataset `name` and starts the next one.  Returns {key: per-picture host values}."""
        done = {}
        for m in self.rows:
            vals, self.vals[m.key] = self.vals[m.key], []
            done[m.key] = m.host(vals, self.opts) if vals else []
            if done[m.key]:
                self.stored[m.key][name] = m.mean(done[m.key], self.opts)
        return done


def single(key, pic, opts, metrics=METRICS):
    """Row `key` of one picture without a target: None when the row is off, NaN when the picture does not count."""
    m = next(m for m in metrics if m.key == key)
    if not m.enabled(opts):
        return None
    host = m.host([m.value(pic, None, opts)], opts) if m.fits(pic, opts) else []
    return m.mean(host, opts) if host else float("nan")


def report_lines(net, model_name, bicubic, always, metrics=METRICS):
    """`<dataset>: [bicubic <side>, ]<model_name> <side>[, <group>]` per dataset of the last test().  <side>: the labels of
    the per_side rows the trainer has a test_<key> of, a missing dataset printing nan; the bicubic side where `bicubic` and
    the dataset has one; a group per other row that stored the dataset.  Nothing unless `always` or there is a group."""
    def have(m, prefix="test_"):
        return getattr(net, prefix + m.key, {})
    sides = [m for m in metrics if m.per_side and hasattr(net, "test_" + m.key)]
    groups = [m for m in metrics if not m.per_side and have(m)]
    lines = []
    for name in have(sides[0]) if always or groups else ():
        parts = [" ".join([model_name] + [m.label % have(m).get(name, float("nan")) for m in sides])]
        if bicubic and name in have(sides[0], "test_bicubic_"):
            parts.insert(0, " ".join(["bicubic"] + [m.label % have(m, "test_bicubic_").get(name, float("nan")) for m in sides]))
        parts += [m.label % have(m)[name] for m in groups if name in have(m)]
        lines.append("%s: %s" % (name, ", ".join(parts)))
    return lines
