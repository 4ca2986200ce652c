"""Trainer objects with the reference's surface — MODEL(args).train() / test() / test_single(fn) /
save_model(epoch) / load_model() — for SRCNN, ESPCN, FSRCNN, VDSR, EDSR, LapSRN, SRGAN and DRCN
(srcnn.py:32-281, espcn.py:32-281, fsrcnn.py:58-307, vdsr.py:39-301, edsr.py:48-351,
lapsrn.py:88-349, srgan.py:93-528, drcn.py:62-355), on the MI355X hot path.

Kept from the reference: per-model hyper-parameters hard-coded in train() (e.g. EDSR base_filter 64 /
16 residuals, edsr.py:87; VDSR momentum 0.9 / wd 1e-4 / clip 0.4, vdsr.py:86-90,149), the epoch-wise
LR decay rules, the checkpoint file names and that checkpoints are weights-only state_dict pickles.
Not kept (out of scope): TF1 logging, plot side effects and the per-iteration host
sync (`loss.data[0]`).  Result pictures are written by test_single(path) and test(save_images=True), with the
colour tail on the device.  Training data comes from a `loader` argument (any iterable of tensor tuples in
the reference's (lr, hr, bicubic) order), else from the reference's image folders under `data_dir`
(data.PatchLoader: decode on host threads, transforms on the GPU) when they exist, else from seeded
synthetic patches of the configured crop size.
"""
import math
import os
import random

import torch

from . import dp as dpmod
from . import evaluation, models, ops, optim, tiling, trainers, utils, video_stream


def synthetic_loader(kind, args, steps, device, seed=1234):
    """Seeded random (input, target...) batches with the shapes each reference train loop feeds."""
    g = torch.Generator().manual_seed(seed)
    b, c, r = args.batch_size, args.num_channels, args.scale_factor
    lr = args.crop_size // r
    hr = lr * r  # the reference crops HR patches to a multiple of the scale (dataset.py calculate_valid_crop_size)
    for _ in range(steps):
        # every reference dataset yields (LR input, HR target) image batches in [0,1] (dataset.py:51-99); the
        # per-model pre-steps (bicubic up/down-sampling, shaving) run on the device in _Trainer.prepare
        if kind == "fsrcnn":            # output r(H-5)+4 = target shaved by 2r (fsrcnn.py:143-150)
            yield torch.rand(b, c, lr, lr, generator=g).to(device), torch.rand(b, c, r * (lr - 5) + 4, r * (lr - 5) + 4, generator=g).to(device)
        elif kind == "vespcn":          # three LR frames [b,3,c,lr,lr] and the centre HR frame (VESPCN.prepare shaves it by 4r)
            yield torch.rand(b, 3, c, lr, lr, generator=g).to(device), torch.rand(b, c, hr, hr, generator=g).to(device)
        elif kind == "espcn":           # net output r(H-8) (the reference's own target is inconsistent, App. B-2)
            yield torch.rand(b, c, lr, lr, generator=g).to(device), torch.rand(b, c, r * (lr - 8), r * (lr - 8), generator=g).to(device)
        else:                           # srcnn / vdsr / lapsrn / edsr / srgan: (lr, hr)
            yield torch.rand(b, c, lr, lr, generator=g).to(device), torch.rand(b, c, hr, hr, generator=g).to(device)


# Epoch-wise learning-rate decay of each reference trainer: kind -> (every N epochs, divide by).  Applied at the top of
# epoch e when (e + 1) % N == 0, to every param group of every optimizer of the trainer.
#   vdsr.py:127-129  /10 every 20     edsr.py:131-133  /2 every 40     lapsrn.py:173-175  /10 every 100
#   srgan.py:239-244 /10 every 20 (G and D)            srcnn.py / espcn.py / fsrcnn.py: no decay
LR_DECAY = {"vdsr": (20, 10.0), "edsr": (40, 2.0), "lapsrn": (100, 10.0), "srgan": (20, 10.0)}
# drcn.py:164-168 /10 every 20 (both param groups).  Kept apart from LR_DECAY, whose content is the seven-trainer table
# the host tests pin; apply_lr_decay reads both.
LR_DECAY_DRCN = {"drcn": (20, 10.0)}


def apply_lr_decay(kind, epoch, *optimizers):
    """The reference's `if (epoch+1) % N == 0: param_group['lr'] /= F` (see LR_DECAY).  Returns True if it decayed."""
    rule = LR_DECAY.get(kind) or LR_DECAY_DRCN.get(kind)
    if rule is None or (epoch + 1) % rule[0] != 0:
        return False
    for opt in optimizers:
        for g in opt.param_groups:
            g['lr'] = g['lr'] / rule[1]
    return True


def _name(args, kind):
    """What a refusal calls the model: args.model_name, else the kind in capitals."""
    return getattr(args, "model_name", None) or kind.upper()


def check_data_flags(args):
    """The loader's degradation flags against each other and against --synthetic."""
    degrade2 = getattr(args, "degrade2", None) is not None      # ({}: --degrade2 with its defaults)
    degrade2_test = getattr(args, "degrade2_test", None) is not None
    flags = [(flag, bool(getattr(args, flag, None))) for flag in ("degrade", "degrade_test", "jpeg_quality", "jpeg_test")]
    for flag, on in flags + [("degrade2", degrade2), ("usm", bool(getattr(args, "usm", False))), ("degrade2_test", degrade2_test)]:
        if on and getattr(args, "synthetic", False):
            raise ValueError("--%s: synthetic patches are not degraded; train and test on image folders (drop --synthetic)"
                             % flag)
    if degrade2 and getattr(args, "degrade", False):
        raise ValueError("--degrade2 and --degrade are two degradation models: give one")
    if degrade2 and getattr(args, "jpeg_quality", None):
        raise ValueError("--jpeg_quality belongs to --degrade; --degrade2's chain has JPEG stages of its own (jpeg_range, "
                         "jpeg_range2 in its settings file)")
    if degrade2_test and (getattr(args, "degrade_test", None) or getattr(args, "jpeg_test", None)):
        raise ValueError("--degrade2_test brings its own blur, noise and JPEG: give neither --degrade_test nor --jpeg_test "
                         "with it")
    if getattr(args, "jpeg_quality", None) and not getattr(args, "degrade", False):
        raise ValueError("--jpeg_quality is a stage of the training degradation: pass --degrade too (--blur_prob 0 "
                         "--noise_sigma 0,0 leaves JPEG alone)")


def check_perceptual_args(args, kind):
    """--vgg_weights / --perceptual / --vgg_loss_weight: the VGG feature term belongs to the SRGAN step, reads RGB, and
    trains only with weights to extract features with.  Raises ValueError naming the flag."""
    perceptual = bool(getattr(args, "perceptual", False))
    vgg_weights = getattr(args, "vgg_weights", None)
    flag = "--perceptual" if perceptual else "--vgg_weights"
    weight = getattr(args, "vgg_loss_weight", None)
    if weight is not None and not 0.0 <= float(weight) < float("inf"):
        raise ValueError("--vgg_loss_weight %r must be a finite number >= 0" % (weight,))
    if (perceptual or vgg_weights) and kind not in ("srgan", "esrgan"):
        raise ValueError("%s: only SRGAN has a VGG feature term, not %s" % (flag, _name(args, kind)))
    if perceptual and not vgg_weights:
        raise ValueError("--perceptual needs --vgg_weights PATH (a torchvision vgg19 state_dict file)")
    if (perceptual or vgg_weights) and getattr(args, "num_channels", 3) != 3:
        raise ValueError("%s: the VGG head reads RGB, use --num_channels 3 (got %r)" % (flag, args.num_channels))


# trainers.mixed_loss's terms (a new one: here and there): flag -> (what a kind without it lacks, the value that leaves it out)
TERM_FLAGS = {"ssim_weight": ("SSIM mix", 0.0), "fft_weight": ("frequency-domain term", 0.0), "fft_norm": (None, "backward"),
              "lpips_weight": ("LPIPS term", 0.0)}


def check_term_args(args, kind, name, flags):
    """The kinds of trainers.OWN_LOSS_KINDS train on losses of their own: a term weight > 0 is refused, naming the flag."""
    for flag in flags:
        weight = getattr(args, flag, 0.0) or 0.0
        if kind in trainers.OWN_LOSS_KINDS and weight > 0:
            raise ValueError("--%s %g: %s has no %s (SRGAN and ESRGAN train on adversarial content terms, DRCN through its "
                             "fused recursive-supervision head); use --%s 0 or another model"
                             % (flag, weight, name, TERM_FLAGS[flag][0], flag))


def check_lpips_args(args, kind):
    """--lpips_vgg / --lpips_lin / --lpips_weight: the two weight files come together, LPIPS reads RGB, and the training
    term belongs to the kinds trainers.mixed_loss serves.  Raises ValueError naming the flag."""
    vgg, lin = getattr(args, "lpips_vgg", None), getattr(args, "lpips_lin", None)
    weight = getattr(args, "lpips_weight", None) or 0.0
    if not 0.0 <= float(weight) < float("inf"):
        raise ValueError("--lpips_weight %r must be a finite number >= 0" % (weight,))
    if bool(vgg) != bool(lin):
        raise ValueError("--lpips_vgg and --lpips_lin come together: LPIPS needs the vgg16 weights and its linear layers")
    if weight > 0 and not vgg:
        raise ValueError("--lpips_weight %g needs --lpips_vgg PATH and --lpips_lin PATH" % weight)
    check_term_args(args, kind, _name(args, kind), ("lpips_weight",))
    if vgg and getattr(args, "num_channels", 3) != 3:
        raise ValueError("--lpips_vgg: LPIPS reads RGB, use --num_channels 3 (got %r; scoring the restored-colour picture "
                         "of a Y model is not supported)" % (args.num_channels,))


def parse_vgg_layers(spec):
    """--vgg_layers: `name:weight,...` or the word `realesrgan` (Real-ESRGAN's five taps, ops.REALESRGAN_VGG_LAYERS), or a
    mapping / pair sequence given in code.  -> ops.vgg_layer_plan's [(name, index, weight)], None for no spec.  ValueError
    naming the culprit."""
    if spec is None:
        return None
    if isinstance(spec, str):
        if spec.strip().lower() == "realesrgan":
            pairs = list(ops.REALESRGAN_VGG_LAYERS)
        else:
            pairs = []
            for item in spec.split(","):
                name, sep, weight = item.strip().partition(":")
                if not sep or not name.strip() or not weight.strip():
                    raise ValueError("vgg_layers: %r is not name:weight (conv1_2:0.1,... or realesrgan)" % (item,))
                pairs.append((name.strip(), weight.strip()))
    else:
        pairs = spec
    return ops.vgg_layer_plan(pairs, models.FeatureExtractor.VGG19_CFG)


def check_vgg_layers_args(args, kind):
    """--vgg_layers belongs to ESRGAN's adversarial phase and needs the VGG19 weights.  Raises ValueError naming the
    flag.  -> the parsed plan, None without the flag."""
    spec = getattr(args, "vgg_layers", None)
    if spec is None:
        return None
    if kind != "esrgan":
        raise ValueError("--vgg_layers: only ESRGAN has the multi-layer VGG feature term, not %s" % _name(args, kind))
    if not getattr(args, "vgg_weights", None):
        raise ValueError("--vgg_layers needs --vgg_weights PATH (a torchvision vgg19 state_dict file)")
    try:
        return parse_vgg_layers(spec)
    except ValueError as e:
        raise ValueError("--vgg_layers %s: %s" % (spec, e))


DISCRIMINATORS = ("vgg", "unet")


def check_discriminator_args(args, kind):
    """--discriminator / --gan_type / --unet_feat belong to ESRGAN's adversarial phase; the relativistic loss takes one
    logit a sample, so it does not go with the U-Net's logit map, whose three stride-2 stages need a crop size that is a
    multiple of 8.  Raises ValueError naming the flag.  -> (discriminator, gan_type, unet_feat) for ESRGAN, the defaults
    of the three filled in (ragan with vgg, vanilla with unet, 64 features)."""
    disc, gan, feat = (getattr(args, n, None) for n in ("discriminator", "gan_type", "unet_feat"))
    if kind != "esrgan":
        for flag, v in (("discriminator", disc), ("gan_type", gan), ("unet_feat", feat)):
            if v is not None:
                raise ValueError("--%s: only ESRGAN chooses its discriminator and GAN loss, not %s" % (flag, _name(args, kind)))
        return None
    disc = disc or "vgg"
    if disc not in DISCRIMINATORS:
        raise ValueError("--discriminator %r is not one of %s" % (disc, ", ".join(DISCRIMINATORS)))
    gan = gan or ("vanilla" if disc == "unet" else "ragan")
    if gan not in trainers.GAN_TYPES:
        raise ValueError("--gan_type %r is not one of %s" % (gan, ", ".join(trainers.GAN_TYPES)))
    if disc == "unet" and gan == "ragan":
        raise ValueError("--gan_type ragan: the relativistic average loss takes one logit a sample, the U-Net discriminator "
                         "gives one a pixel (use --gan_type vanilla with --discriminator unet)")
    if feat is not None and disc != "unet":
        raise ValueError("--unet_feat: only the U-Net discriminator has a feature count to set (pass --discriminator unet)")
    if feat is not None and int(feat) < 1:
        raise ValueError("--unet_feat %r must be a whole number >= 1" % (feat,))
    crop = getattr(args, "crop_size", None)
    if disc == "unet" and crop is not None and int(crop) % 8:
        raise ValueError("--crop_size %d is not a multiple of 8, which the three stride-2 stages of --discriminator unet need"
                         % int(crop))
    return disc, gan, 64 if feat is None else int(feat)


# VESPCN's own flags and their defaults (None on the command line: the default; set with another model: refused by name)
VESPCN_FLAGS = {"mc_weight": 0.01, "flow_weight": 0.001, "vespcn_max_flow": 8.0}


def check_one_gpu(name):
    """ESRGAN and DRCN: no data parallelism (WORLD_SIZE is what torch.distributed.run sets)."""
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise NotImplementedError("%s trains on one GPU (a world size of %s): data parallelism is not implemented for it "
                                  "(launch main.py without torch.distributed.run)" % (name, os.environ["WORLD_SIZE"]))


def check_growth(flag, growth):
    """--rdn_growth / --rrdb_growth: what the slice convolutions of a dense block can write."""
    if growth % 16 or growth > 64:
        raise ValueError("--%s %d: the slice convolutions write 16, 32, 48 or 64 channels" % (flag, growth))


def discriminator_kind(state_dict):
    """'unet' or 'vgg' from the keys of a discriminator's state_dict."""
    return "unet" if any(k.endswith("weight_orig") for k in state_dict) else "vgg"


# -- the training-state file (<save_dir>/model/<model_name>_train_state.pkl) ---------------------------------------------
# Everything a run needs to continue at an epoch boundary as if it had not stopped; plain containers, numbers, strings
# and CPU tensors only, so it loads with torch.load(weights_only=True).  The weights-only checkpoint files beside it are
# the reference's and do not change.
STATE_VERSION = 1


def check_resume_state(state, model_name, num_channels, scale_factor):
    """A state file continues only the kind of run that wrote it.  ValueError names the field that differs."""
    if not isinstance(state, dict) or state.get("version") != STATE_VERSION:
        raise ValueError("version: not a training-state file of format %d (%r)"
                         % (STATE_VERSION, state.get("version") if isinstance(state, dict) else type(state).__name__))
    for field, mine in (("model_name", model_name), ("num_channels", num_channels), ("scale_factor", scale_factor)):
        if state.get(field) != mine:
            raise ValueError("%s: the training state was written for %r, this run has %r (main.py --%s)"
                             % (field, state.get(field), mine, field))


def _cpu_state(module):
    return {k: v.detach().cpu().clone() for k, v in module.state_dict().items()}


def _ema_name(name):
    """The EMA weights' file beside a checkpoint file: `_ema` in front of `.pkl`."""
    return name[:-len('.pkl')] + '_ema.pkl'


def _option(args, name, value=None, default=None):
    """A per-call option: the argument, else args.<name> where the args object has such a field, else `default`."""
    if value is None:
        value = getattr(args, name, None)
    return default if value is None else value


class _Trainer(object):
    kind = None
    decay_kind = property(lambda self: self.kind)   # whose LR_DECAY rule lr_decay applies; a subclass names another kind's
    pre_upsample = False     # the net takes the bicubic-upsampled picture (SRCNN, VDSR, DRCN)
    edsr_ckpt_name = False   # checkpoint files named as edsr.py:324-337 (ch / batch / epoch / lr), not as srcnn.py:260-269
    HYPER = {}               # the model's hyper-parameter flags and their defaults
    VGG_LOSS_WEIGHT = 6e-3   # --vgg_loss_weight's default (srgan.py:306)

    @classmethod
    def hyper(cls, args):
        """{flag: args.<flag>, else its default} for cls.HYPER's flags, for args objects with and without the field."""
        return {flag: getattr(args, flag, None) or default for flag, default in cls.HYPER.items()}

    @classmethod
    def check_flags(cls, args):
        """Every rule about which flags go with this model and with each other, on the host: the one place main.py's
        usage errors and a trainer built from code take them from.  The rules common to all models are here (the check_*
        helpers); a subclass puts its own in front and calls this.  Raises ValueError naming the flag as the user types
        it.  -> (the parsed --vgg_layers plan or None, ESRGAN's (discriminator, gan_type, unet_feat) or None)."""
        name = _name(args, cls.kind)
        check_term_args(args, cls.kind, name, ("ssim_weight", "fft_weight"))
        fft, crop = getattr(args, "fft_weight", None) or 0.0, getattr(args, "crop_size", None)
        if fft > 0 and crop is not None and crop > 256:
            raise ValueError("--fft_weight %g: the dense DFT takes HR patches of at most 256 on a side, --crop_size is %d"
                             % (fft, crop))
        check_perceptual_args(args, cls.kind)
        check_lpips_args(args, cls.kind)      # (lpips_weight is refused there, between the checks of its files)
        vgg_layers = check_vgg_layers_args(args, cls.kind)
        disc_args = check_discriminator_args(args, cls.kind)
        if getattr(args, "net_interp", None) is not None and cls.kind != "esrgan":
            raise ValueError("--net_interp: only ESRGAN has a pre-trained and an adversarial generator to blend, not %s" % name)
        for flag in VESPCN_FLAGS:
            if getattr(args, flag, None) is not None and cls.kind != "vespcn":
                raise ValueError("--%s: only VESPCN has a motion-compensation stage, not %s" % (flag, name))
        check_data_flags(args)
        optim._check_ema_decay(getattr(args, "ema_decay", 0.0))
        return vgg_layers, disc_args

    @classmethod
    def flag_defaults(cls, args):
        """{flag: value} of the flags whose default depends on the model or on another flag, for accepted args."""
        weight = getattr(args, "vgg_loss_weight", None)
        return {"vgg_loss_weight": cls.VGG_LOSS_WEIGHT if weight is None else float(weight)}

    def __init__(self, args):
        self.vgg_layers, self.disc_args = type(self).check_flags(args)
        # the reference copies args field by field (edsr.py:49-65)
        for k in ("model_name", "train_dataset", "test_dataset", "crop_size", "num_threads", "num_channels",
                  "scale_factor", "num_epochs", "save_epochs", "batch_size", "test_batch_size", "lr", "data_dir",
                  "save_dir", "gpu_mode"):
            setattr(self, k, getattr(args, k, None))
        self.args = args
        self.steps_per_epoch = getattr(args, "steps_per_epoch", 8)
        self.ema_decay = optim._check_ema_decay(getattr(args, "ema_decay", 0.0))
        self.resume = getattr(args, "resume", None)
        self.use_ema = bool(getattr(args, "use_ema", False))
        if not torch.cuda.is_available():
            raise RuntimeError("the MI355X hot path needs a GPU (gpu_mode=False has no CPU fallback; see oracle/)")
        self.rank, self.world, self.local = dpmod.init_from_env()
        torch.cuda.set_device(self.local)
        self.device = torch.device("cuda", self.local)
        self.model = None

    # -- overridables --------------------------------------------------------------------------
    def build_model(self):
        raise NotImplementedError

    def lr_decay(self, epoch, *optimizers):
        apply_lr_decay(self.decay_kind, epoch, *optimizers)

    def build_step(self):
        """(flat parameters, optimizer, DataParallel or None, eager step function) of the freshly built model."""
        terms = {flag: getattr(self.args, flag, None) or off for flag, (_, off) in TERM_FLAGS.items()}
        return trainers.build(self.kind, self.model, self.lr, use_dp=self.world > 1, ema_decay=self.ema_decay,
                              lpips_net=self.lpips_net(), **terms)

    def lpips_net(self):
        """models.LPIPS with the weights of --lpips_vgg / --lpips_lin on this trainer's device, built once; None without
        the two files."""
        if getattr(self, "_lpips", None) is None and getattr(self.args, "lpips_vgg", None):
            net = models.LPIPS().load_vgg16(self.args.lpips_vgg).load_lins(self.args.lpips_lin)
            self._lpips = net.to(self.device).eval()
        return getattr(self, "_lpips", None)

    def niqe_params(self):
        """(mu_p, cov_p) of --niqe_params (utils.load_niqe_params), read once; None without the flag."""
        if getattr(self, "_niqe", None) is None and getattr(self.args, "niqe_params", None):
            self._niqe = utils.load_niqe_params(self.args.niqe_params)
        return getattr(self, "_niqe", None)

    def _ensure_model(self):
        if self.model is None:
            self.model = self.build_model().to(self.device)
            self.load_model()

    # -- training state: save at epoch boundaries, continue with --resume --------------------------------------------
    def _state_name(self):
        model_dir = os.path.join(self.save_dir, 'model')
        os.makedirs(model_dir, exist_ok=True)
        return model_dir + '/' + self.model_name + '_train_state.pkl'

    def _optimizers(self):
        """{name in the state file: optimizer}."""
        return {"optimizer": self.optimizer}

    def _modules(self):
        """{name in the state file: module}."""
        return {"model": self.model}

    def training_state(self, done, history, loader=None, **extra):
        """The state after `done` completed epochs (see STATE_VERSION)."""
        rnd = random.getstate()
        state = {"version": STATE_VERSION, "model_name": self.model_name, "num_channels": self.num_channels,
                 "scale_factor": self.scale_factor, "epochs_done": int(done),
                 "batch_size": self.batch_size, "lr": self.lr, "world": self.world,
                 "history": [list(h) if isinstance(h, tuple) else h for h in history],
                 "modules": {k: _cpu_state(m) for k, m in self._modules().items()},
                 "optimizers": {k: o.state_dict() for k, o in self._optimizers().items()},
                 "python_random": [rnd[0], list(rnd[1]), rnd[2]],
                 "torch_rng": torch.get_rng_state().clone()}
        if hasattr(loader, "state_dict") and hasattr(loader, "load_state_dict"):
            state["loader"] = loader.state_dict()
        state.update(extra)
        return state

    def _write_state(self, state):
        """Atomically: a run killed while it writes leaves the previous file."""
        name = self._state_name()
        torch.save(state, name + '.tmp')
        os.replace(name + '.tmp', name)

    def save_state(self, done, history, loader=None, **extra):
        if self.rank == 0:
            self._write_state(self.training_state(done, history, loader, **extra))

    def read_resume_state(self):
        """None without `resume`; else the checked state of the file it names ('auto': this run's own)."""
        if not self.resume:
            return None
        name = self._state_name() if self.resume == 'auto' else os.fspath(self.resume)
        if not os.path.exists(name):
            raise FileNotFoundError("--resume: no training state at %r" % (name,))
        state = torch.load(name, map_location="cpu", weights_only=True)
        check_resume_state(state, self.model_name, self.num_channels, self.scale_factor)
        return state

    def load_training_state(self, state, loader=None):
        """Into the freshly built model and optimizers, in place (under data parallelism after the broadcast: every rank
        reads the same file).  Returns (completed epochs, history so far)."""
        for k, m in self._modules().items():
            m.load_state_dict(state["modules"][k])     # (FlatParams' post-hook marks the flat buffer changed)
        for k, o in self._optimizers().items():
            o.load_state_dict(state["optimizers"][k])
        rnd = state["python_random"]
        random.setstate((rnd[0], tuple(rnd[1]), rnd[2]))
        torch.set_rng_state(state["torch_rng"])
        if "loader" in state and hasattr(loader, "load_state_dict"):
            loader.load_state_dict(state["loader"])
        changed = ["%s %r -> %r" % (f, state.get(f), mine) for f, mine in
                   (("batch_size", self.batch_size), ("lr", self.lr), ("world", self.world)) if state.get(f) != mine]
        if self.rank == 0:
            stored = next(iter(self._optimizers().values())).param_groups[0]["lr"]
            print("Resumed after epoch %d%s" % (state["epochs_done"], "" if not changed else
                  " (%s; the stored learning rate %g is used)" % (", ".join(changed), stored)))
        return int(state["epochs_done"]), list(state["history"])

    def begin_epoch(self, epoch):
        """Top of every epoch, before its first step: the reference's LR decay of every optimizer (and any per-model
        schedule)."""
        self.lr_decay(epoch, *self._optimizers().values())

    def _shave(self, target):
        """The part of a target the net's output covers: all of it, but for SRCNN."""
        return target

    def prepare(self, inp, target):
        """(input, target) of the data loader -> the tensors the train step consumes, on the device:
          SRCNN   y = img_interp(input, r) (bicubic), x = shave(target, 8)               (srcnn.py:116-125; its override)
          VDSR    y = img_interp(input, r), x = target                 (vdsr.py:133-142; drcn.py:183-190 alike)
          LapSRN  y = input, x_coarse = img_interp(target, 1/r*2), x_finer = target       (lapsrn.py:179-188; its override)
        utils.img_interp is the bit-exact GPU form of the reference's per-image PIL loop."""
        return self._net_input(inp), target

    def load_dataset(self, dataset, is_train=True):
        """edsr.py:67-84 / srgan.py:110-129: the image-folder loaders of data.py behind the reference's directory layout
        (data_dir/<dataset>/..., DIV2K_train_LR_bicubic/X4 for DIV2K), as data.PatchLoader (decode on host threads,
        uint8 over PCIe through pinned memory, every transform on the GPU).  Under data parallelism every rank draws the
        same per-epoch permutation and takes its own 1/world of it (PatchLoader rank / world).
        A missing or empty TRAINING folder raises, as the reference's DataLoader would -- unless the run asked for
        seeded synthetic patches (`--synthetic`), in which case None is returned.  Missing TEST folders return None:
        test() evaluates the test sets that exist (the reference's list names three)."""
        from . import data
        is_gray = self.num_channels == 1
        synthetic = bool(getattr(self.args, "synthetic", False))
        if synthetic:
            return None
        args = self.args
        try:
            if is_train:
                degrade = None
                if getattr(args, "degrade", False):   # main.py --degrade: LR = (HR * k) shrunk + n (data.Degradation)
                    degrade = data.Degradation(blur_prob=getattr(args, "blur_prob", 1.0),
                                               blur_sigma=getattr(args, "blur_sigma", (0.2, 4.0)),
                                               noise_sigma=getattr(args, "noise_sigma", (0.0, 10.0)),
                                               jpeg_quality=getattr(args, "jpeg_quality", None),
                                               jpeg_prob=getattr(args, "jpeg_prob", 1.0),
                                               jpeg_subsampling=getattr(args, "jpeg_subsampling", "420"))
                if getattr(args, "degrade2", None) is not None:   # main.py --degrade2: the second-order chain
                    degrade = data.Degradation2(**dict(args.degrade2))
                ds = data.get_training_set(self.data_dir, dataset, self.crop_size, self.scale_factor, is_gray=is_gray,
                                           device=self.device, degrade=degrade, usm=bool(getattr(args, "usm", False)))
                bs, shuffle = self.batch_size, True
            else:
                fixed = getattr(args, "degrade_test", None)   # (s1, s2, theta in degrees, noise sigma)
                if fixed:
                    fixed = (fixed[0], fixed[1], math.radians(fixed[2]), fixed[3])
                seed2 = getattr(args, "degrade2_test", None)   # every test item under its own seeded chain
                if seed2 is not None:
                    settings = getattr(args, "degrade2", None) or {}
                    seed2 = (data.Degradation2(**dict(settings)), int(seed2))
                ds = data.get_test_set(self.data_dir, dataset, self.scale_factor, is_gray=is_gray, device=self.device,
                                       degrade=fixed or None, jpeg=getattr(args, "jpeg_test", None),
                                       jpeg_subsampling=getattr(args, "jpeg_subsampling", "420"), degrade2=seed2)
                bs, shuffle = self.test_batch_size or 1, False
        except (OSError, TypeError) as e:
            if not is_train:
                return None
            raise FileNotFoundError("training set %r not found under --data_dir %r (%s: %s); pass --synthetic to train on "
                                    "seeded random patches instead" % (dataset, self.data_dir, type(e).__name__, e))
        if len(ds) == 0:
            if not is_train:
                return None
            raise FileNotFoundError("training set %r under --data_dir %r holds no images; pass --synthetic to train on "
                                    "seeded random patches instead" % (dataset, self.data_dir))
        if is_train:   # DP: disjoint 1/world shards of one common permutation per epoch
            return data.PatchLoader(ds, bs, shuffle=shuffle, num_threads=self.num_threads or 4, seed=1234,
                                    rank=self.rank, world=self.world)
        return data.PatchLoader(ds, bs, shuffle=shuffle, num_threads=self.num_threads or 4)

    def open_data(self, loader):
        """The training batches of train(): `loader`, else the image folders, else None (seeded synthetic patches); says
        which on rank 0."""
        self.data_source = "loader"
        if loader is None:
            loader = self.load_dataset(self.train_dataset, is_train=True)
            self.data_source = "folder" if loader is not None else "synthetic"
        if self.rank == 0:
            print("training data: %s%s" % (self.data_source, "" if self.data_source != "folder" else
                                           " %s under %s" % (self.train_dataset, self.data_dir)))
        return loader

    def _channels(self, *tensors):
        """num_channels == 1: only the Y channel is super-resolved (edsr.py:139-142: hr[:, 0].unsqueeze(1))."""
        if self.num_channels == 1:
            return tuple(t[..., :1, :, :].contiguous() if t.shape[-3] != 1 else t for t in tensors)   # (the channel axis of pictures and clips)
        return tensors

    # -- reference surface ------------------------------------------------------------------------
    def train(self, loader=None, log_every=0):
        state = self.read_resume_state()
        self.model = self.build_model()
        self.model.weight_init()
        self.model.to(self.device).train()
        utils.print_network(self.model) if self.rank == 0 else None
        self.flat, self.optimizer, self.dp, step = self.build_step()
        loader = self.open_data(loader)
        done, avg_loss = (0, []) if state is None else self.load_training_state(state, loader)
        trainers.quiesce_gc()    # no full cyclic collection (~80 ms) inside a step from here on

        def batches(epoch):
            for batch in loader if loader is not None else synthetic_loader(self.kind, self.args, self.steps_per_epoch,
                                                                            self.device, 1234 + epoch * self.world + self.rank):
                inp, target = self._channels(*[t.to(self.device, non_blocking=True) for t in batch][:2])
                yield self.prepare(inp, target)

        def one_loss(*tensors):
            out = self._step(step, tensors)
            return sum(out) if isinstance(out, tuple) else out

        self.run_epochs(done, self.num_epochs, batches, one_loss, 1, avg_loss, 'Epoch: [%2d] avg loss: %.8f', self.begin_epoch,
                        lambda n: (self.save_model(n), self.save_state(n, avg_loss, loader)))
        self._close_graph()
        if self.rank == 0:
            self.save_model(epoch=None)
            self.save_state(max(done, self.num_epochs), avg_loss, loader)
        return avg_loss

    def run_epochs(self, first, last, batches, step, losses=0, history=None, line=None, begin=None, save=None):
        """Epochs first .. last - 1 of one training phase: begin(epoch), then step(*tensors) for every item of
        batches(epoch).  The first `losses` values a step returns are summed on the device (no host sync inside the loop)
        and read once per epoch: their means go to `history` (a float, or a tuple of several) and on rank 0 into `line`.
        Every save_epochs epochs rank 0 calls save(epochs done)."""
        for epoch in range(first, last):
            if begin is not None:
                begin(epoch)
            totals, n = [torch.zeros((), device=self.device) for _ in range(losses)], 0
            for tensors in batches(epoch):
                out = step(*tensors)
                for total, loss in zip(totals, out if isinstance(out, tuple) else (out,)):
                    total += loss.detach()
                n += 1
            if losses:
                means = tuple(float(total) / max(n, 1) for total in totals)   # one sync per epoch
                history.append(means if losses > 1 else means[0])
            if self.rank == 0:
                if line is not None:
                    print(line % ((epoch + 1,) + means))
                if save is not None and (epoch + 1) % self.save_epochs == 0:
                    save(epoch + 1)

    # -- the train step as a hipGraph ------------------------------------------------------------------------------
    # The reference's loop launches ~110 (EDSR) small kernels per iteration; at its default batch sizes the step is a
    # few hundred microseconds of GPU work behind 1.5+ ms of host launches.  The FIRST batch of a shape runs eagerly (a
    # real training step, and every lazy initialisation happens outside a capture), the next one is captured
    # (trainers.capture_step: zero_grad + filter packing + forward + loss + backward + optimizer as one graph, split at
    # the gradient exchange under data parallelism) and replayed from then on.  A batch of another shape (the ragged
    # last one) runs eagerly; a learning-rate decay needs nothing (the rate is a device scalar).  --eager turns it off.
    # A step without segments (LapSRN's two losses, DRCN) cannot be split: it is captured on one GPU only.
    def auto_graph(self, eager_step, flats, enabled=True):
        return trainers.AutoGraph(eager_step, lambda ts: trainers.capture_step(eager_step, ts, warmup=0, flats=flats),
                                  enabled=enabled and not getattr(self.args, "eager", False))

    def _step(self, eager_step, tensors):
        auto = getattr(self, "_auto", None)
        if auto is None or auto.eager is not eager_step:
            single = self.dp is None or not self.dp.active
            auto = self._auto = self.auto_graph(eager_step, [self.flat], hasattr(eager_step, "segments") or single)
        return auto(*tensors)

    @property
    def _graph(self):
        auto = getattr(self, "_auto", None)
        return None if auto is None else auto.graph

    def _close_graph(self):
        auto = getattr(self, "_auto", None)
        if auto is not None:
            auto.close()

    def _net_input(self, x):
        """SRCNN / VDSR feed the bicubic-upsampled image to the net (srcnn.py:145, vdsr.py:160)."""
        return utils.img_interp(x, self.scale_factor) if self.pre_upsample else x

    def _infer(self, x):
        self.model.eval()
        with torch.no_grad():
            return self.model(x.to(self.device))

    def _net(self, x):
        """_infer, the last element of a tuple output."""
        y = self._infer(x)
        return y[-1] if isinstance(y, tuple) else y

    @staticmethod
    def _chroma_at(chroma, oh, ow):
        """(cb, cr): the 8-bit chroma planes [2,h,w] resized to oh x ow, both in one resizer call; (None, None) without."""
        return (None, None) if chroma is None else tuple(ops.resize_u8(chroma, int(oh), int(ow)))

    # -- tiled inference (tiling.py, csrc/tile.hip) ------------------------------------------------------------------
    def _resolve_tile(self, tile, x, ensemble=False):
        """The `tile` option (_option) for the net input x -> (tile size or None for one pass, the net's geometry or None;
        nothing is computed without the option).  ensemble: the geometry is the union of the net's cone and its mirror image."""
        tile = _option(self.args, 'tile', tile)
        if tile is None:
            return None, None
        self.model.eval()
        geo = tiling.net_geometry(self.model)
        if ensemble:
            geo = tiling.ensemble_geometry(geo)
        return tiling.resolve_tile(tile, geo, int(x.shape[-2]), int(x.shape[-1])), geo

    # -- x8 geometric self-ensemble (csrc/dihedral.hip) ---------------------------------------------------------------
    def _self_ensemble(self, flag):
        """The `self_ensemble` option: None falls back to args.self_ensemble (older args objects have no such field: off)."""
        return bool(_option(self.args, 'self_ensemble', flag, False))

    def _infer_variants(self, x):
        """The net (last element of a tuple output) on the eight variants T_k, k = 4 m + r, T_k = rot90(flip of the last
        axis if m, r), of the net inputs x [N,C,H,W]: one launch makes all of them, the net runs on the four of the
        picture's shape and on the four of the transposed shape (as ONE batch of 8 N when the pictures are square).
        Returns (even, odd): the outputs for k = 0, 2, 4, 6 and for k = 1, 3, 5, 7, what ops.dihedral_merge takes."""
        var = ops.dihedral_variants(x)
        if var.whole is not None:
            y = self._net(var.whole)
            even, odd = y[:y.shape[0] // 2], y[y.shape[0] // 2:]
        else:
            even, odd = self._net(var.even), self._net(var.odd)
        if tuple(odd.shape) != (even.shape[0], even.shape[1], even.shape[3], even.shape[2]):
            raise RuntimeError("self-ensemble: the net returned %s for the pictures and %s for the transposed ones; it must "
                               "treat both axes alike" % (tuple(even.shape), tuple(odd.shape)))
        return even, odd

    def _infer_tiled(self, x, geo, tile, tile_batch=None, as_u8=False, chroma=None, ensemble=False):
        """The net's output for the net input x [1,C,H,W] (on the device), computed on overlapping tiles: the plan's table
        goes to the device once, then per chunk of `tile_batch` tiles: k_tile_gather -> _infer on the batch (last element
        of a tuple output) -> k_tile_stitch of the rectangles those tiles own.  The peak working set is one chunk's
        activations plus the output picture; nothing waits for the device.  Returns the fp32 picture [1,C,OH,OW], or with
        as_u8 the final interleaved 8-bit picture (chroma: the picture's 8-bit Cb / Cr planes [2,h,w], resized here to the
        output size and merged by the stitch), in which case the fp32 picture is never written.
        ensemble (geo is then tiling.ensemble_geometry of the net's): every chunk goes gather -> the eight variants of its
        tiles -> net -> k_dihedral_merge to the fp32 tile outputs -> the same stitch; `tile_batch` then counts net inputs,
        variants included, rounded up to whole tiles (tiling.tiles_per_chunk)."""
        plan = tiling.plan(geo, int(x.shape[-2]), int(x.shape[-1]), tile)
        tp = ops.TilePlan(plan, self.device)
        tile_batch = tiling.tiles_per_chunk(_option(self.args, 'tile_batch', tile_batch), plan.ntiles, ensemble)
        cb, cr = self._chroma_at(chroma, plan.OH, plan.OW)
        out = None
        for t0 in range(0, plan.ntiles, tile_batch):
            tiles = ops.tile_gather(x, tp, t0, min(tile_batch, plan.ntiles - t0))
            y = ops.dihedral_merge(*self._infer_variants(tiles)) if ensemble else self._net(tiles)
            if tuple(y.shape[-2:]) != (plan.oth, plan.otw):
                raise RuntimeError("tiled inference: the net returned %s for a tile of %d x %d, the geometry says %d x %d"
                                   % (tuple(y.shape), plan.th, plan.tw, plan.oth, plan.otw))
            if as_u8:
                out = ops.tile_stitch_u8(y, tp, t0, out, cb, cr)
            else:
                out = ops.tile_stitch(y, tp, t0, out)
        return out if as_u8 else out.unsqueeze(0)

    def _run(self, x, tile, tile_batch, ens, as_u8=False, chroma=None):
        """The net -- or with `ens` its x8 geometric ensemble (see test_single) -- on the net input x [1,C,H,W]: tiled when
        `tile` says so, else in one pass.  Returns the fp32 output, or with as_u8 the final interleaved 8-bit picture, written
        by the last kernel of the path (chroma: the picture's 8-bit Cb / Cr planes [2,h,w] of a Y model, resized to the
        size the net returned and merged there)."""
        size, geo = self._resolve_tile(tile, x, ens)
        if size is not None:
            return self._infer_tiled(x, geo, size, tile_batch, as_u8, chroma, ens)
        if ens:
            even, odd = self._infer_variants(x)
            if not as_u8:
                return ops.dihedral_merge(even, odd)
            return ops.dihedral_merge_u8(even, odd, *self._chroma_at(chroma, even.shape[-2], even.shape[-1]))
        out = self._net(x)
        if not as_u8:
            return out
        if chroma is None:
            return ops.to_u8_image(out)
        return ops.ycbcr_to_rgb_u8(out, *self._chroma_at(chroma, out.shape[-2], out.shape[-1]))

    def _forward(self, x, tile=None, tile_batch=None, self_ensemble=None):
        """_net_input and the net (last element of a tuple output) on the device: one pass, or tiled when `tile` says so;
        with self_ensemble the x8 geometric ensemble of the net (see test_single) in place of the net."""
        return self._run(self._net_input(x), tile, tile_batch, self._self_ensemble(self_ensemble))

    def test(self, loader=None, save_images=False, tile=None, eval_domain=None, eval_shave=None, self_ensemble=None):
        """Evaluation loop (espcn.py:173-215, edsr.py:196-250): the net on every picture of `loader`, else of every folder
        of `test_dataset` that exists under `data_dir`, else of seeded synthetic pairs, and the rows of evaluation.METRICS
        of its output against the target, on the device.  Returns the PSNRs, one per picture whose output has the target's
        shape; `self.test_<key>[dataset]` holds the per-dataset numbers of every row that is on (the table says what a row
        is, when it is on and which pictures it leaves out; DESIGN.md section 36 which attributes a call creates).
        save_images: as edsr.py:215-274, every result also goes through utils.save_img into <save_dir>/test_result/
        <dataset>/SR_result_<n>.png, and the rows of the loader's bicubic picture (the third item, where there is one)
        against the unshaved target go to `self.test_bicubic_<key>`.  tile / self_ensemble: as test_single takes them.
        eval_domain / eval_shave: None (the args object's), or the domain and border of the `eval` row; NIQE shaves the same
        border.  Nothing inside the loop reads a device value back (utils.save_img's copy of the picture apart)."""
        self._ensure_model()
        opts = evaluation.Options(self, _option(self.args, 'eval_domain', eval_domain), _option(self.args, 'eval_shave', eval_shave))
        mine, returned = evaluation.Scores(self, opts), []
        bicubic = evaluation.Scores(self, opts, bicubic=True) if save_images else None
        for name, batches in self._test_sources(loader):
            img_num = 0
            for batch in batches:
                items = [batch] if torch.is_tensor(batch[0]) else list(zip(*batch))   # ragged test images come as lists
                for item in items:
                    lr_img, hr_img = self._channels(*[t if t.dim() >= 4 else t.unsqueeze(0) for t in item[:2]])   # (5-D: a batch of clips)
                    out = self._forward(lr_img.to(self.device), tile, self_ensemble=self_ensemble)
                    hr = hr_img.to(self.device)
                    mine.add(out, self._shave(hr))   # (srcnn.py:193-199: border excluded)
                    if save_images:
                        img_num += 1
                        utils.save_img(out[0], img_num, save_dir=os.path.join(self.save_dir, 'test_result', str(name)))
                        if len(item) > 2:
                            bc_img = self._channels(item[2] if item[2].dim() == 4 else item[2].unsqueeze(0))[0]
                            bicubic.add(bc_img.to(self.device), hr)
            returned += mine.finish(name)[evaluation.RETURNED]
            if bicubic is not None:
                bicubic.finish(name)
        return returned

    def _test_sources(self, loader):
        """[(dataset name, iterable of batches)] of test(): `loader`, else the test sets on disk, else synthetic pairs."""
        if loader is not None:
            return [("loader", loader)]
        found = [(n, self.load_dataset(n, is_train=False)) for n in (self.test_dataset or []) if isinstance(n, str) and len(n) > 1]
        return [s for s in found if s[1] is not None] or [("synthetic", synthetic_loader(self.kind, self.args, 2, self.device, 4321))]

    def test_single(self, img, tile=None, tile_batch=None, self_ensemble=None):
        """A tensor: super-resolve one [C,H,W] (or [1,C,H,W]) tensor and return the net's output on the host.
        A path (str / os.PathLike): the reference's test_single(img_fn) (edsr.py:276-322) -- super-resolve the picture
        file, write <save_dir>/test_result/SR_result.png and return that file name; see _test_single_file.
        tile: None (args.tile, else off) runs the picture in one pass, as a batch of one.  A number cuts the net's input
        (the bicubic-upsampled picture for SRCNN / VDSR / DRCN) into overlapping tiles of that many pixels a side, runs
        them in batches of `tile_batch` (tiling.DEFAULT_TILE_BATCH; 'all' = one batch) and stitches every output pixel
        from the one tile that holds its whole receptive field: the one-pass result, with a working set that does not
        grow with the picture.  'auto' tiles only pictures whose widest activation exceeds tiling.AUTO_BUDGET_BYTES.
        self_ensemble: None (args.self_ensemble, else off) or a bool.  On: the geometric self-ensemble of the EDSR paper
        ("EDSR+") in place of the net f: with T_k(x) = rot90(flip of the last axis if m, r turns), k = 4 m + r, the result
        is (((((((y_0 + y_1) + y_2) + y_3) + y_4) + y_5) + y_6) + y_7) * 0.125 in fp32, y_k = T_k^-1(f(T_k(x))).  It wraps
        the net, not the pre-processing (the bicubic picture of SRCNN / VDSR / DRCN is made once and transformed), and with
        num_channels == 1 not the chroma.  The variants and the mean are one kernel launch each (csrc/dihedral.hip); the
        path form's mean is written as the 8-bit picture.  Tiled, the plan allows for the mirrored net's dependency cone
        (tiling.ensemble_geometry) and `tile_batch` counts net inputs, variants included."""
        if isinstance(img, (str, os.PathLike)):
            return self._test_single_file(img, tile, tile_batch, self_ensemble)
        self._ensure_model()
        x = img if img.dim() == 4 else img.unsqueeze(0)
        return self._forward(x.to(self.device), tile, tile_batch, self_ensemble).cpu()

    def _test_single_file(self, img_fn, tile=None, tile_batch=None, self_ensemble=None):
        """edsr.py:276-322 with the picture on the device from the decode to the 8-bit result:
          num_channels == 1  upload the 8-bit RGB once -> k_rgb_to_ycc (fp32 Y / 255 and planar Cb / Cr in one pass) -> Y
                             through _net_input and _infer exactly as the tensor form does (bicubic pre-upsampling for
                             SRCNN / VDSR / DRCN, last element of a tuple output) -> Cb and Cr through the 8-bit bicubic
                             resizer (one call, two planes) to the height and width the net actually returned (FSRCNN
                             and ESPCN crop a border) -> k_ycc_to_rgb (quantises Y on the way) -> one device-to-host
                             copy of the 8-bit image;
          num_channels == 3  RGB / 255 in, k_to_u8 out.
        Bit-exact with the reference's Pillow tail for the same net output.  Nothing between the upload and that copy
        waits for the device.  Tiled (see test_single): the stitch kernel writes the 8-bit result itself (k_tile_stitch
        quantises, and merges the resized chroma, on the way), so the fp32 HR picture never exists.  Every trainer follows
        the EDSR convention for the net's output, clamp(0, 1): SRCNN's own test_single stretches the output to its min..max
        instead (srcnn.py:244), which turns any picture grey-scaled to full range; that is not reproduced.
        self_ensemble (see test_single): k_dihedral_merge writes the 8-bit picture from the eight outputs (it quantises, and
        merges the resized chroma, on the way); tiled, it writes the fp32 tile outputs the stitch then reads."""
        from . import data
        self._ensure_model()
        rgb = torch.tensor(data.load_img(os.fspath(img_fn)), device=self.device)   # [H,W,3] uint8: the one upload
        h, w = int(rgb.shape[0]), int(rgb.shape[1])
        chroma = None
        if self.num_channels == 1:
            y, chroma = ops.rgb_to_ycc_planes(rgb, y_float=True)
            x = y.view(1, 1, h, w)
        else:
            x = ops.resize_u8(rgb.permute(2, 0, 1), h, w, out_float=True).unsqueeze(0)   # ToTensor: planar, / 255
        ens = self._self_ensemble(self_ensemble)
        img8 = self._run(self._net_input(x), tile, tile_batch, ens, as_u8=True, chroma=chroma)
        # NIQE of the very bytes the file gets (the colour-restored picture of a Y model), where --niqe_params asks for it
        niqe = evaluation.single("niqe", img8, evaluation.Options(self, eval_shave=_option(self.args, 'eval_shave')))
        if niqe is not None:
            self.test_single_niqe = niqe
        return self._save_single(img8)

    def _save_single(self, img8):
        from PIL import Image
        arr = img8.cpu().numpy()   # the one device-to-host copy
        result_dir = os.path.join(self.save_dir, 'test_result')
        os.makedirs(result_dir, exist_ok=True)
        save_fn = result_dir + '/SR_result.png'
        Image.fromarray(arr).save(save_fn)
        print('Single test result image is saved.')
        return save_fn

    # -- raw video streams (data.Y4MReader / Y4MWriter, csrc/video.hip) -------------------------------------------------
    VIDEO_RADIUS = 0   # frames on either side of frame t that the net looks at for output frame t (video_stream)

    def _video_net(self, tile, tile_batch, ens):
        """The net of test_video, video_stream.run's callable: the unpacked slot x and (lo, n) -> the fp32 output for
        the frames x[lo : lo + n].  tile (the option, resolved) / ens: frame by frame through the existing one-picture
        path in its fp32 form, with its refusals."""
        if ens or tile is not None:
            return lambda x, lo, n: torch.cat([self._run(self._net_input(x[j:j + 1]), tile, tile_batch, ens) for j in range(lo, lo + n)])
        return lambda x, lo, n: self._net(self._net_input(x[lo:lo + n]))

    def test_video(self, src, dst=None, batch=None, tile=None, tile_batch=None, self_ensemble=None):
        """Super-resolve a YUV4MPEG2 stream (8-bit 4:2:0, 4:4:4 or mono, progressive): src / dst are a path, '-' (stdin /
        stdout) or a binary file object; dst None: <save_dir>/test_result/SR_result.y4m.  Returns the number of frames.
        Frames go in batches of `batch` (args.video_batch, else 8; the last may be short) from file bytes to file bytes on
        the device: k_yuv_unpack (num_channels 1: Y / 255; 3: RGB through Pillow's tables, 4:2:0 chroma bicubic to full
        size first) -> _net_input and the net on the whole batch -> k_yuv_pack (num_channels 1: Y' quantised, Cb / Cr of
        the input through the 8-bit bicubic resizer to the chroma size of what the net returned; 3: Pillow's RGB -> YCbCr
        and for 4:2:0 its BOX shrink of the chroma, fused).  Samples are full-range JFIF values; the chroma resampling is
        centre-aligned whatever the C tag says, and the tag is carried through.
        The pipeline is video_stream.run, the same for every trainer: reader and writer threads, three streams, every
        buffer made once.  A trainer gives it VIDEO_RADIUS (output frame t is the net on frames max(t - R, 0) ..
        min(t + R, T - 1) of the stream, as many frames out as in; a Y model's chroma comes from frame t) and _video_net.
        tile / tile_batch / self_ensemble as test_single: with either, frames go one at a time through _run, with its
        refusals.  dst '-': everything this call prints goes to stderr.  A caller that sets self.video_trace to a list gets
        torch.cuda.memory_allocated() appended at the end of every batch."""
        import contextlib
        import sys
        if isinstance(dst, (str, os.PathLike)) and os.fspath(dst) == '-':
            # stdout carries the stream and nothing else: whatever this call prints (load_model's line, the frame count)
            # goes to stderr
            sink = sys.stdout.buffer
            with contextlib.redirect_stdout(sys.stderr):
                return self.test_video(src, sink, batch, tile, tile_batch, self_ensemble)
        self._ensure_model()
        net = self._video_net(_option(self.args, 'tile', tile), tile_batch, self._self_ensemble(self_ensemble))
        n_max = int(_option(self.args, 'video_batch', batch, 8))
        if n_max <= 0:
            raise ValueError("test_video: batch must be positive (got %d)" % n_max)
        if dst is None:
            dst = os.path.join(self.save_dir, 'test_result', 'SR_result.y4m')
        frames, lay, out_lay, dt = video_stream.run(src, dst, n_max, self.VIDEO_RADIUS, net, self.num_channels, self.device,
                                                    getattr(self, 'video_trace', None))
        print('Video: %d frames -> %d x %d (%s), %.1f frames/s' % (frames, out_lay.W, out_lay.H, lay.sub, frames / dt))
        return frames

    def _ckpt_name(self, epoch):
        # srcnn.py:260-269 style for the simple trainers, edsr.py:324-337 style (ch/batch/epoch/lr) for EDSR / SRGAN
        model_dir = os.path.join(self.save_dir, 'model')
        os.makedirs(model_dir, exist_ok=True)
        if self.edsr_ckpt_name:
            return model_dir + '/' + self.model_name + '_param_ch%d_batch%d_epoch%d_lr%.g.pkl' % (
                self.num_channels, self.batch_size, self.num_epochs if epoch is None else epoch, self.lr)
        if epoch is not None:
            return model_dir + '/' + self.model_name + '_param_epoch_%d.pkl' % epoch
        return model_dir + '/' + self.model_name + '_param.pkl'

    def save_model(self, epoch=None):
        sd = {k: v.detach().cpu().clone() for k, v in self.model.state_dict().items()}
        torch.save(sd, self._ckpt_name(epoch))
        if self.ema_decay > 0:   # the EMA weights beside it: the same keys and shapes, a file load_model() reads alike
            self._save_ema(self.optimizer, self.model, self._ckpt_name(epoch))
        print('Trained model is saved.')

    @staticmethod
    def _save_ema(opt, module, name):
        torch.save({k: v.detach().cpu().clone() for k, v in opt.ema_state_dict(module).items()}, _ema_name(name))

    def load_model(self):
        name = self._ckpt_name(None)
        if self.use_ema:
            name = _ema_name(name)
            if not os.path.exists(name):
                print('No EMA model exists to load (%s).' % os.path.basename(name))
                return False
        if os.path.exists(name):
            self.model.load_state_dict(torch.load(name))
            print('Trained model is loaded.')
            return True
        print('No model exists to load.')
        return False


class SRCNN(_Trainer):
    kind = "srcnn"
    pre_upsample = True

    def build_model(self):
        return models.SRCNNNet(self.num_channels, 64)   # srcnn.py:73

    def _shave(self, target):
        return utils.shave(target, 8)

    def prepare(self, inp, target):
        return self._net_input(inp), self._shave(target).contiguous()


class ESPCN(_Trainer):
    kind = "espcn"

    def build_model(self):
        return models.ESPCNNet(self.num_channels, 64, self.scale_factor)   # espcn.py:73


class FSRCNN(_Trainer):
    kind = "fsrcnn"

    def build_model(self):
        return models.FSRCNNNet(self.num_channels, self.scale_factor, 56, 12, 4)   # fsrcnn.py:99


class VDSR(_Trainer):
    kind = "vdsr"
    pre_upsample = True

    def build_model(self):
        return models.VDSRNet(self.num_channels, 64, 18)   # vdsr.py:80


class EDSR(_Trainer):
    kind = "edsr"
    edsr_ckpt_name = True

    def build_model(self):
        return models.EDSRNet(self.num_channels, 64, 16)   # edsr.py:87


class LapSRN(_Trainer):
    kind = "lapsrn"

    def build_model(self):
        return models.LapSRNNet(self.num_channels, 64, 10)   # lapsrn.py:129

    def prepare(self, inp, target):
        return inp, utils.img_interp(target, 1 / self.scale_factor * 2), target


class SRGAN(_Trainer):
    """srgan.py:93-528: generator pre-training with MSE, then the adversarial loop."""
    kind = "srgan"
    opt_kinds = ("srgan_g", "srgan_d")

    def _normalise(self, t):
        """What the loader's batches go through on their way to both phases (srgan.py:193-194,257-258)."""
        return utils.norm(t, vgg=True)

    def _pretrain_step(self, g_opt, g_dp):
        """The generator's pre-training step (srgan.py:179-219: MSE)."""
        return trainers.mse_step(self.G, g_opt, g_dp)

    def _adversarial_step(self, g_opt, d_opt, g_dp, d_dp):
        """The adversarial step (two models, two optimizers); data parallel: cut at the two exchanges.
        --vgg_weights: the reference's VGG content term in the logged G loss; --perceptual: the term trains G."""
        fe = None
        if getattr(self.args, "vgg_weights", None):
            fe = models.FeatureExtractor().load_vgg19(self.args.vgg_weights).to(self.device)
        return trainers.srgan_step(self.G, self.D, g_opt, d_opt, g_dp, d_dp, feature_extractor=fe, lazy_pack=True,
                                   prune_dead_grads=bool(getattr(self.args, "prune_dead_grads", False)),
                                   perceptual=bool(getattr(self.args, "perceptual", False)),
                                   vgg_weight=self.flag_defaults(self.args)["vgg_loss_weight"])

    def build_model(self):
        self.G = models.SRGANGenerator(self.num_channels, 64, 16)                 # srgan.py:136
        self.D = models.SRGANDiscriminator(self.num_channels, 64, self.crop_size)  # srgan.py:137
        return self.G

    def _optimizers(self):
        return {"g_opt": self.g_opt, "d_opt": self.d_opt}

    def _modules(self):
        return {"G": self.G, "D": self.D}

    def train(self, loader=None, pretrain_epochs=None, log_every=0):
        state = self.read_resume_state()
        self.model = self.build_model()
        self.G.weight_init(mean=0.0, std=0.02)
        self.D.weight_init(mean=0.0, std=0.02)
        self.G.to(self.device).train()
        self.D.to(self.device).train()
        g_flat, d_flat = optim.FlatParams(self.G), optim.FlatParams(self.D)
        g_opt = self.g_opt = optim.make_optimizer(self.opt_kinds[0], g_flat, self.lr, ema_decay=self.ema_decay)   # (the EMA is G's)
        d_opt = self.d_opt = optim.make_optimizer(self.opt_kinds[1], d_flat, self.lr)
        g_dp = d_dp = None
        if self.world > 1:
            g_dp, d_dp = dpmod.DataParallel(g_flat), dpmod.DataParallel(d_flat)
            g_dp.broadcast_params()
            d_dp.broadcast_params()
            g_opt.ema_reset()
            if getattr(self.args, "sync_bn", False):   # statistics of the global batch (SURVEY.md 8e caveat)
                trainers.sync_batchnorm(self.G)
                trainers.sync_batchnorm(self.D)
        norm = self._normalise
        loader = self.open_data(loader)
        trainers.quiesce_gc()    # no full cyclic collection (~80 ms) inside a step from here on

        def batches(seed):   # loaders yield (lr, hr) or the reference's (lr, hr, bicubic) tuples (dataset.py:101)
            for batch in (loader or synthetic_loader("srgan", self.args, self.steps_per_epoch, self.device, seed)):
                lr_img, hr_img = self._channels(*batch[:2])
                yield norm(lr_img.to(self.device, non_blocking=True)), norm(hr_img.to(self.device, non_blocking=True))

        # generator pre-training (srgan.py:179-219): 50 epochs of MSE unless a pre-trained generator checkpoint loads
        self.epoch_pretrain = int(getattr(self.args, "epoch_pretrain", 50)) if pretrain_epochs is None else pretrain_epochs
        # a resumed run continues in the phase it stopped in: inside pre-training after `pre_done` of its epochs, or in the
        # adversarial loop after `done` epochs with the history so far
        self.phase, pre_done, done, hist = "pretrain", 0, 0, []
        if state is not None:
            self.phase = state["phase"]
            n, h = self.load_training_state(state, loader)
            if self.phase == "pretrain":
                pre_done = n
            else:
                done, hist = n, [tuple(v) for v in h]
        if self.phase == "adversarial":
            pass
        elif state is None and self.load_model(is_pretrain=True):
            g_flat.mark_changed()      # parameters changed behind the optimizer's back: re-pack filters
            g_opt.ema_reset()          # ... and the shadow weights start from them
        else:
            pre_step = self.auto_graph(self._pretrain_step(g_opt, g_dp), [g_flat])
            self.run_epochs(pre_done, self.epoch_pretrain, lambda epoch: batches(77 + epoch), pre_step, save=lambda n:
                            n < self.epoch_pretrain and self.save_state(n, [], loader, phase="pretrain"))
            pre_step.close()
            if self.rank == 0:
                self.save_model(is_pretrain=True)
        if self.phase == "pretrain":
            self.phase = "adversarial"
            self.save_state(0, [], loader, phase=self.phase)
        # the adversarial step (two models, two optimizers) as one hipGraph; data parallel: graphs split at the two exchanges
        step = self.auto_graph(self._adversarial_step(g_opt, d_opt, g_dp, d_dp), [g_flat, d_flat])
        self.run_epochs(done, self.num_epochs, lambda epoch: batches(1234 + epoch), step, 2, hist,
                        'Epoch: [%2d] D_loss: %.8f G_loss: %.8f', self.begin_epoch,   # srgan.py:239-244: both rates decay
                        lambda n: (self.save_model(n), self.save_state(n, hist, loader, phase=self.phase)))
        step.close()
        if self.rank == 0:
            self.save_model(epoch=None)
            self.save_state(max(done, self.num_epochs), hist, loader, phase=self.phase)
        return hist

    def _names(self, epoch):
        model_dir = os.path.join(self.save_dir, 'model')
        os.makedirs(model_dir, exist_ok=True)
        tail = '_param_ch%d_batch%d_epoch%d_lr%.g.pkl' % (self.num_channels, self.batch_size,
                                                           self.num_epochs if epoch is None else epoch, self.lr)
        return (model_dir + '/' + self.model_name + '_G' + tail, model_dir + '/' + self.model_name + '_D' + tail,
                model_dir + '/' + self.model_name + '_G_param_pretrain.pkl')

    def save_model(self, epoch=None, is_pretrain=False):   # srgan.py:483-506
        g_name, d_name, pre = self._names(epoch)
        cpu = lambda m: {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
        if is_pretrain:
            torch.save(cpu(self.G), pre)
            if self.ema_decay > 0:
                self._save_ema(self.g_opt, self.G, pre)
            print('Pre-trained generator model is saved.')
        else:
            torch.save(cpu(self.G), g_name)
            torch.save(cpu(self.D), d_name)
            if self.ema_decay > 0:   # (the generator's only)
                self._save_ema(self.g_opt, self.G, g_name)
            print('Trained models are saved.')

    def load_model(self, is_pretrain=False):   # srgan.py:508-526
        g_name, _, pre = self._names(None)
        name = pre if is_pretrain else g_name
        if self.use_ema and not is_pretrain:   # (what test() / test_single() evaluate; train() starts from the plain file)
            name = _ema_name(name)
            if not os.path.exists(name):
                print('No EMA generator model exists to load (%s).' % os.path.basename(name))
                return False
        if os.path.exists(name):
            self.G.load_state_dict(torch.load(name))
            print('Trained generator model is loaded.')
            return True
        return False


class ESRGAN(SRGAN):
    """ESRGAN (Wang et al., ECCV-W 2018; not in the reference collection) on SRGAN's two-phase trainer: models.RRDBNet
    (`--rrdb_blocks` blocks of growth `--rrdb_growth`, 64 trunk channels) pre-trained with L1 for `--epoch_pretrain` epochs
    into the same `_G_param_pretrain.pkl`, then trainers.esrgan_step against models.ESRGANDiscriminator with
    `--pixel_weight` * L1 + `--vgg_loss_weight` * the conv5_4 feature L1 + `--gan_weight` * the relativistic average loss;
    both optimizers Adam at --lr, no learning-rate decay rule of its own.  Batches stay in [0, 1] (the feature term
    normalises once).  x4 only; one GPU; `--tile` is refused (the exact halo of 23 blocks is about 350 LR pixels: the
    tiles would be mostly halo); `--net_interp A` evaluates (1 - A) * the pre-trained + A * the adversarial generator."""
    kind = "esrgan"
    opt_kinds = ("esrgan_g", "esrgan_d")
    decay_kind = None
    HYPER = {"rrdb_blocks": 23, "rrdb_growth": 32}
    VGG_LOSS_WEIGHT = 1.0

    @classmethod
    def check_flags(cls, args):
        if getattr(args, "scale_factor", 4) != 4:
            raise ValueError("--scale_factor %r: RRDBNet upsamples by 4 only" % (args.scale_factor,))
        if getattr(args, "tile", None) is not None:
            raise ValueError("--tile: the RRDB trunk reaches about 350 LR pixels to each side (23 blocks), a tile would be "
                             "mostly halo; ESRGAN's pictures run in one pass (drop --tile)")
        check_growth("rrdb_growth", int(cls.hyper(args)["rrdb_growth"]))
        if getattr(args, "num_channels", 3) != 3:
            raise ValueError("--num_channels %r: ESRGAN's VGG feature term reads RGB, use --num_channels 3" % (args.num_channels,))
        if getattr(args, "perceptual", False):
            raise ValueError("--perceptual: ESRGAN's feature term always trains the generator (drop --perceptual)")
        interp = getattr(args, "net_interp", None)
        if interp is not None and not 0.0 <= float(interp) <= 1.0:
            raise ValueError("--net_interp %r is not in [0, 1]" % (interp,))
        check_one_gpu("ESRGAN")
        return super(ESRGAN, cls).check_flags(args)

    @classmethod
    def flag_defaults(cls, args):
        disc, gan, feat = check_discriminator_args(args, cls.kind)
        return dict(super(ESRGAN, cls).flag_defaults(args), discriminator=disc, gan_type=gan,
                    unet_feat=feat if disc == "unet" else None)

    def __init__(self, args):
        super(ESRGAN, self).__init__(args)
        self.blocks, self.growth = (int(v) for v in self.hyper(args).values())
        w = lambda name, default: default if getattr(args, name, None) is None else float(getattr(args, name))
        self.gan_weight, self.pixel_weight = w("gan_weight", 5e-3), w("pixel_weight", 1e-2)
        self.vgg_weight = self.flag_defaults(args)["vgg_loss_weight"]
        self.net_interp = None if getattr(args, "net_interp", None) is None else float(args.net_interp)
        self.discriminator, self.gan_type, self.unet_feat = self.disc_args

    def build_discriminator(self):
        """--discriminator vgg (default): SRGAN's body ending in a logit; unet: Real-ESRGAN's UNetDiscriminatorSN."""
        if self.discriminator == "unet":
            return models.UNetDiscriminatorSN(self.num_channels, self.unet_feat)
        return models.ESRGANDiscriminator(self.num_channels, 64, self.crop_size)

    def build_model(self):
        self.G = models.RRDBNet(self.num_channels, 64, self.blocks, self.growth, self.scale_factor)
        self.D = self.build_discriminator()
        return self.G

    def load_training_state(self, state, loader=None):
        stored = discriminator_kind(state["modules"]["D"])
        mine = discriminator_kind(self.D.state_dict())
        if stored != mine:
            raise ValueError("discriminator: the training state holds a %r discriminator, this run builds a %r one "
                             "(main.py --discriminator %s)" % (stored, mine, stored))
        return super(ESRGAN, self).load_training_state(state, loader)

    def _normalise(self, t):
        return t

    def _pretrain_step(self, g_opt, g_dp):
        return trainers.l1_step(self.G, g_opt, g_dp)

    def _adversarial_step(self, g_opt, d_opt, g_dp, d_dp):
        layers = self.vgg_layers
        deepest = 34 if layers is None else max(idx for _, idx, _ in layers)
        fe = models.FeatureExtractor(feature_layer=deepest).load_vgg19(self.args.vgg_weights).to(self.device)
        return trainers.esrgan_step(self.G, self.D, g_opt, d_opt, fe, self.pixel_weight, self.vgg_weight, self.gan_weight,
                                    self.gan_type, None if layers is None else [(name, w) for name, _, w in layers])

    def train(self, loader=None, pretrain_epochs=None, log_every=0):
        if not getattr(self.args, "vgg_weights", None):
            raise ValueError("--vgg_weights PATH is required: ESRGAN's adversarial phase trains on VGG19 conv5_4 features (a "
                             "torchvision vgg19 state_dict file)")
        return super(ESRGAN, self).train(loader, pretrain_epochs, log_every)

    def load_model(self, is_pretrain=False):
        """The generator's checkpoint; with net_interp A (evaluation only) the blend (1 - A) * pre-trained + A * adversarial
        of the two files, made on the device by srk_axpby.  A missing file is an error that names it."""
        if is_pretrain or self.net_interp is None:
            return super(ESRGAN, self).load_model(is_pretrain)
        g_name, _, pre = self._names(None)
        if self.use_ema:
            g_name = _ema_name(g_name)
        for name in (pre, g_name):
            if not os.path.exists(name):
                raise FileNotFoundError("--net_interp: no generator checkpoint at %r" % (name,))
        a = self.net_interp
        theta_pre = torch.load(pre, map_location="cpu")
        theta_gan = torch.load(g_name, map_location="cpu")
        blend = {}
        for k, v in self.G.state_dict().items():
            p, q = theta_pre[k].to(self.device).contiguous(), theta_gan[k].to(self.device).contiguous()
            blend[k] = ops._axpby(p, q, 1.0 - a, a) if v.is_floating_point() else q
        self.G.load_state_dict(blend)
        print('Interpolated generator model is loaded (%g of the adversarial one).' % a)
        return True


class DRCN(_Trainer):
    """drcn.py:62-355: F = 256 and D = 16 hard-coded as in the reference (drcn.py:103-104); Adam over two param groups
    (the model, w) at the same rate; alpha decays from 1 by 1/25 at the top of every epoch, beta = 1e-3."""
    kind = "drcn"
    pre_upsample = True
    base_filter, num_recursions = 256, 16

    @classmethod
    def check_flags(cls, args):
        check_one_gpu("DRCN")
        checked = super(DRCN, cls).check_flags(args)
        if float(getattr(args, "ema_decay", None) or 0.0) > 0:
            raise ValueError("--ema_decay %g: DRCN keeps no EMA of its weights (its combine weights w train outside the flat "
                             "parameter buffer); use --ema_decay 0 or another model" % args.ema_decay)
        return checked

    def __init__(self, args):
        super(DRCN, self).__init__(args)
        self.loss_alpha = 1.0
        self.loss_alpha_zero_epoch = 25
        self.loss_alpha_decay = self.loss_alpha / self.loss_alpha_zero_epoch
        self.loss_beta = 0.001

    def build_model(self):
        return models.DRCNNet(self.num_channels, self.base_filter, self.num_recursions)

    def next_alpha(self):
        """drcn.py:171: the iterated `loss_alpha = max(0, loss_alpha - loss_alpha_decay)` of the top of every epoch."""
        self.loss_alpha = max(0.0, self.loss_alpha - self.loss_alpha_decay)
        return self.loss_alpha

    def build_step(self):
        """Adam over the model's flat buffer and over w (drcn.py:108-111), alpha and the weight-decay value as device
        scalars the (captured) head reads; the base loop replays the step as one graph (trainers.capture_step)."""
        self.flat = optim.FlatParams(self.model)
        self.optimizer = optim.make_optimizer("drcn", self.flat, self.lr)
        self.w_optimizer = optim.TensorAdam(self.model.w, self.lr)
        self.alpha_dev = torch.ones((), dtype=torch.float32, device=self.device)
        self.reg_dev = torch.zeros((), dtype=torch.float32, device=self.device)
        self.loss_alpha = 1.0
        step = trainers.drcn_step(self.model, self.optimizer, self.w_optimizer, self.alpha_dev, self.loss_beta,
                                  self.reg_dev)
        return self.flat, self.optimizer, None, step

    def _optimizers(self):   # (both param groups decay: drcn.py:164-168)
        return {"optimizer": self.optimizer, "w_optimizer": self.w_optimizer}

    def training_state(self, done, history, loader=None, **extra):
        return super(DRCN, self).training_state(done, history, loader, w=self.model.w.detach().cpu().clone(),
                                                loss_alpha=float(self.loss_alpha), **extra)

    def load_training_state(self, state, loader=None):
        out = super(DRCN, self).load_training_state(state, loader)
        with torch.no_grad():
            self.model.w.copy_(state["w"].reshape(self.model.w.shape))
        self.loss_alpha = float(state["loss_alpha"])   # (begin_epoch takes the next value from here)
        return out

    def begin_epoch(self, epoch):
        super(DRCN, self).begin_epoch(epoch)
        self.alpha_dev.fill_(self.next_alpha())     # drcn.py:171, read by the (captured) head kernel

    def _w_name(self, epoch):
        model_dir = os.path.join(self.save_dir, 'model')
        os.makedirs(model_dir, exist_ok=True)
        if epoch is not None:
            return model_dir + '/' + self.model_name + '_w_epoch_%d.pkl' % epoch
        return model_dir + '/' + self.model_name + '_w.pkl'

    def save_model(self, epoch=None):   # drcn.py:327-339
        super(DRCN, self).save_model(epoch)
        torch.save(self.model.w.detach().cpu().clone(), self._w_name(epoch))

    def load_model(self):   # drcn.py:341-355: the parameters and w, each if its file exists
        loaded = super(DRCN, self).load_model()
        name = self._w_name(None)
        if os.path.exists(name):
            w = torch.load(name)
            with torch.no_grad():
                self.model.w.copy_(w.reshape(self.model.w.shape))
            print('Trained weight is loaded.')
        else:
            print('No weight exists to load.')
        return loaded


class RCAN(_Trainer):
    """RCAN (models.RCANNet; not in the reference collection) behind the common trainer: L1 and Adam as EDSR, EDSR's
    learning-rate decay, `--rcan_groups` x `--rcan_blocks` RCABs with `--rcan_reduction`.  Its channel attention reads the
    whole picture, so tiling is refused here (args.tile) and by tiling.net_geometry (test_single(img, tile=...))."""
    kind = "rcan"
    decay_kind = "edsr"
    HYPER = {"rcan_groups": 10, "rcan_blocks": 20, "rcan_reduction": 16}

    @classmethod
    def check_flags(cls, args):
        if getattr(args, "tile", None) is not None:
            raise ValueError("--tile: RCAN's channel attention depends on the whole image, its pictures run in one pass "
                             "(drop --tile)")
        if 64 % int(cls.hyper(args)["rcan_reduction"]):
            raise ValueError("--rcan_reduction %d does not divide RCAN's 64 channels" % args.rcan_reduction)
        if getattr(args, "scale_factor", 4) not in (2, 4, 8):
            raise ValueError("--scale_factor %r: RCAN upsamples by 2, 4 or 8" % (args.scale_factor,))
        return super(RCAN, cls).check_flags(args)

    def __init__(self, args):
        super(RCAN, self).__init__(args)
        self.groups, self.blocks, self.reduction = (int(v) for v in self.hyper(args).values())

    def build_model(self):
        return models.RCANNet(self.num_channels, 64, self.groups, self.blocks, self.reduction, self.scale_factor)


class RDN(_Trainer):
    """RDN (models.RDNNet; not in the reference collection) behind the common trainer: L1 and Adam as EDSR, EDSR's
    learning-rate decay, `--rdn_blocks` residual dense blocks of `--rdn_layers` layers with growth `--rdn_growth`, 64
    shallow features.  Purely convolutional: `--tile` works (tiling.net_geometry)."""
    kind = "rdn"
    decay_kind = "edsr"
    HYPER = {"rdn_blocks": 16, "rdn_layers": 8, "rdn_growth": 64}

    @classmethod
    def check_flags(cls, args):
        check_growth("rdn_growth", int(cls.hyper(args)["rdn_growth"]))
        if getattr(args, "scale_factor", 4) not in (2, 3, 4):
            raise ValueError("--scale_factor %r: RDN upsamples by 2, 3 or 4" % (args.scale_factor,))
        return super(RDN, cls).check_flags(args)

    def __init__(self, args):
        super(RDN, self).__init__(args)
        self.blocks, self.layers, self.growth = (int(v) for v in self.hyper(args).values())

    def build_model(self):
        return models.RDNNet(self.num_channels, 64, self.blocks, self.layers, self.growth, self.scale_factor)


class SwinIR(_Trainer):
    """SwinIR (models.SwinIRNet; not in the reference collection) behind the common trainer: L1 and Adam as EDSR, EDSR's
    learning-rate decay; `--swinir_dim`, `--swinir_depths`, `--swinir_heads`, `--swinir_window`, `--swinir_mlp_ratio`,
    `--swinir_upsampler`.  The window grid and the border mask of its WindowAttention belong to the whole picture, so
    tiling is refused here (args.tile) and by tiling.net_geometry (test_single(img, tile=...))."""
    kind = "swinir"
    decay_kind = "edsr"
    HYPER = {"swinir_dim": 180, "swinir_depths": (6, 6, 6, 6, 6, 6), "swinir_heads": 6, "swinir_window": 8,
             "swinir_mlp_ratio": 2, "swinir_upsampler": "pixelshuffle"}

    @classmethod
    def check_flags(cls, args):
        h = cls.hyper(args)
        dim, heads, window, upsampler = int(h["swinir_dim"]), int(h["swinir_heads"]), int(h["swinir_window"]), h["swinir_upsampler"]
        scale, crop = getattr(args, "scale_factor", None), getattr(args, "crop_size", None)
        if getattr(args, "tile", None) is not None:
            raise ValueError("--tile: SwinIR's WindowAttention partitions the whole image into windows, its pictures run in "
                             "one pass (drop --tile)")
        if dim % heads:
            raise ValueError("--swinir_heads %d does not divide --swinir_dim %d" % (heads, dim))
        if dim // heads > 32:
            raise ValueError("--swinir_dim %d / --swinir_heads %d: a head dimension of %d exceeds 32" % (dim, heads, dim // heads))
        if not 2 <= window <= 8:
            raise ValueError("--swinir_window %d is not in 2 .. 8" % window)
        if upsampler == "pixelshuffle" and scale is not None and scale not in (2, 3, 4, 8):
            raise ValueError("--scale_factor %d: SwinIR's pixelshuffle upsampler works by 2, 3, 4 or 8" % scale)
        if scale and crop is not None and (crop % scale or (crop // scale) % window):
            raise ValueError("--crop_size %d / --scale_factor %d is not a multiple of --swinir_window %d" % (crop, scale, window))
        return super(SwinIR, cls).check_flags(args)

    def __init__(self, args):
        super(SwinIR, self).__init__(args)
        dim, depths, heads, window, mlp_ratio, self.upsampler = self.hyper(args).values()
        self.dim, self.heads, self.window, self.mlp_ratio = int(dim), int(heads), int(window), float(mlp_ratio)
        self.depths = tuple(int(d) for d in (depths.split(",") if isinstance(depths, str) else depths))

    def build_model(self):
        return models.SwinIRNet(self.num_channels, self.dim, self.depths, self.heads, self.window, self.mlp_ratio,
                                self.scale_factor, self.upsampler)


class VESPCN(_Trainer):
    """VESPCN (models.VESPCNNet; not in the reference collection) behind the common trainer: three LR frames in, the
    super-resolved centre frame out; MSE + `--mc_weight` * motion-compensation MSE + `--flow_weight` * flow smoothness
    on Adam, ESPCN's optimizer rule (trainers.build("vespcn")); `--vespcn_max_flow`.  Batches are (frames [B,3,C,h,w],
    centre HR frame); the target is shaved by 4 r, what the valid trunk leaves.  A single picture (test_single, test() on
    picture folders) is its own neighbours: the flow net then sees three equal frames.  One GPU."""
    kind = "vespcn"
    HYPER = VESPCN_FLAGS

    @classmethod
    def check_flags(cls, args):
        if getattr(args, "tile", None) is not None:
            raise ValueError("--tile: VESPCN's MotionCompensator warps by a learned flow of up to 1.25 --vespcn_max_flow "
                             "pixels, its pictures run in one pass (drop --tile)")
        if getattr(args, "self_ensemble", False):
            raise ValueError("--self_ensemble: a flipped or rotated clip is not run for VESPCN (its flow has a direction); "
                             "drop --self_ensemble")
        check_one_gpu("VESPCN")
        for flag in ("degrade", "degrade_test", "degrade2", "degrade2_test", "usm", "jpeg_quality", "jpeg_test"):
            v = getattr(args, flag, None)
            if v is not None and v is not False:
                raise ValueError("--%s: VESPCN's clips are shrunk by the clean bicubic only; the degradations are per-picture "
                                 "and not built for three frames" % flag)
        for flag in ("ssim_weight", "fft_weight", "lpips_weight"):
            if (getattr(args, flag, 0.0) or 0.0) > 0:
                raise ValueError("--%s %g: VESPCN trains on MSE + motion compensation + flow smoothness and has no %s; use "
                                 "--%s 0" % (flag, getattr(args, flag), TERM_FLAGS[flag][0], flag))
        h = cls.hyper(args)
        if not float(h["vespcn_max_flow"]) > 0.0:
            raise ValueError("--vespcn_max_flow %r is not positive" % (args.vespcn_max_flow,))
        scale, crop = getattr(args, "scale_factor", None) or 4, getattr(args, "crop_size", None)   # (main.py's default scale)
        if crop is not None and (crop // scale) % 4:
            raise ValueError("--crop_size %d / --scale_factor %d = %d is not a multiple of 4, which the two stride-2 stages "
                             "of VESPCN's flow net need" % (crop, scale, crop // scale))
        return super(VESPCN, cls).check_flags(args)

    @classmethod
    def hyper(cls, args):
        return {flag: default if getattr(args, flag, None) is None else getattr(args, flag) for flag, default in cls.HYPER.items()}

    def __init__(self, args):
        super(VESPCN, self).__init__(args)
        h = self.hyper(args)
        self.mc_weight, self.flow_weight, self.max_flow = float(h["mc_weight"]), float(h["flow_weight"]), float(h["vespcn_max_flow"])

    def build_model(self):
        return models.VESPCNNet(self.num_channels, 64, self.scale_factor, self.max_flow)

    def build_step(self):
        return trainers.build(self.kind, self.model, self.lr, use_dp=False, ema_decay=self.ema_decay,
                              mc_weight=self.mc_weight, flow_weight=self.flow_weight)

    def load_dataset(self, dataset, is_train=True):
        """Clip folders, data_dir/<dataset>/<clip>/<frames>, through data.PatchLoader: data.ClipDataset for training,
        data.ClipTestDataset for test(); None with --synthetic."""
        from . import data
        if not is_train:
            # a test set of clip folders: every frame with its neighbours (the ends use themselves); a folder of pictures
            # goes through the picture loader, each picture its own neighbours
            root = os.path.join(self.data_dir or "", dataset)
            if bool(getattr(self.args, "synthetic", False)) or not os.path.isdir(root):
                return None
            if not any(os.path.isdir(os.path.join(root, d)) for d in os.listdir(root)):
                return super(VESPCN, self).load_dataset(dataset, is_train)
            ds = data.get_clip_test_set(self.data_dir, dataset, self.scale_factor, is_gray=self.num_channels == 1,
                                        device=self.device)
            return data.PatchLoader(ds, 1, shuffle=False, num_threads=self.num_threads or 4) if len(ds) else None
        if bool(getattr(self.args, "synthetic", False)):
            return None
        try:
            ds = data.get_clip_training_set(self.data_dir, dataset, self.crop_size, self.scale_factor,
                                            is_gray=self.num_channels == 1, device=self.device)
        except (OSError, TypeError) as e:
            raise FileNotFoundError("training clips %r not found under --data_dir %r (%s: %s); pass --synthetic to train on "
                                    "seeded random clips instead" % (dataset, self.data_dir, type(e).__name__, e))
        if len(ds) == 0:
            raise FileNotFoundError("training set %r under --data_dir %r holds no clip folder of three or more frames; pass "
                                    "--synthetic to train on seeded random clips instead" % (dataset, self.data_dir))
        return data.PatchLoader(ds, self.batch_size, shuffle=True, num_threads=self.num_threads or 4, seed=1234)

    def _shave(self, target):
        return utils.shave(target, 4 * self.scale_factor)

    def prepare(self, inp, target):
        return self._net_input(inp), self._shave(target).contiguous()

    def _net_input(self, x):
        """A clip [N,3,C,H,W] as it is; pictures [N,C,H,W] as their own neighbours."""
        return x if x.dim() == 5 else x.unsqueeze(1).expand(-1, 3, -1, -1, -1).contiguous()

    VIDEO_RADIUS = 1

    def _video_net(self, tile, tile_batch, ens):
        """The [n,3,C,H,W] windows of the unpacked slot (one strided copy) through the net; tile and self_ensemble are
        refused, as check_flags refuses them."""
        if ens or tile is not None:
            raise ValueError("test_video: VESPCN runs its frames in one pass, without --tile and --self_ensemble")
        return lambda x, lo, n: self._net(torch.stack([x[lo - 1:lo - 1 + n], x[lo:lo + n], x[lo + 1:lo + 1 + n]], 1))


TRAINERS = {"SRCNN": SRCNN, "VDSR": VDSR, "ESPCN": ESPCN, "FSRCNN": FSRCNN, "SRGAN": SRGAN, "LapSRN": LapSRN, "EDSR": EDSR,
            "DRCN": DRCN, "RCAN": RCAN, "RDN": RDN, "SwinIR": SwinIR, "ESRGAN": ESRGAN}
# The nets that take clips, [N,3,C,H,W], instead of pictures: a table of their own beside the twelve picture models.
# trainer_class(name) and model_names() are what main.py asks.
VIDEO_TRAINERS = {"VESPCN": VESPCN}


def model_names():
    return list(TRAINERS) + list(VIDEO_TRAINERS)


def trainer_class(name):
    """The trainer class of --model_name `name`, from either table."""
    return TRAINERS[name] if name in TRAINERS else VIDEO_TRAINERS[name]
