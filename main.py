#!/usr/bin/env python3
"""Entry point with the reference's command line (main.py:13-36: the same 15 flags and defaults)
dispatching to the MI355X trainers.  Extra flags: --synthetic (seeded random patches instead of the image
folders under --data_dir; --steps_per_epoch of them per epoch), --epoch_pretrain, --precision {mixed,bf16x3,fp32},
--test_single PATH (load the checkpoint, super-resolve that picture file into <save_dir>/test_result/SR_result.png, print
the file name; no training) and --save_test_images (test() also writes every result image and reports the bicubic PSNR) and --tile N|auto (--test_single
and test() cut the picture into overlapping tiles, run them as batches and stitch the exact result), --test_only (load
the checkpoint and run test() on the test sets, no training; one line per dataset with PSNR and SSIM) and --eval_domain
{float,u8,y8} / --eval_shave N (test() also reports PSNR and SSIM on the 8-bit picture or its luma, with a border left out)
and --self_ensemble (--test_single, --test_only and the test() after training run every picture through the x8 geometric
self-ensemble, "EDSR+": the net on the eight flips / rotations, transformed back and averaged) and --ssim_weight A (train
on (1 - A) * the model's pixel loss + A * (1 - SSIM), A in [0, 1], default 0; every model but SRGAN and DRCN; the logged
loss is the mixed one) and --fft_weight W (add W * the L1 on the 2-D Fourier spectrum of prediction - target, ops.fft_loss, to that
loss; W >= 0, default 0; --fft_norm {backward,ortho}; HR patches of at most 256 on a side; not SRGAN and DRCN) and --vgg_weights PATH (SRGAN: a torchvision vgg19 state_dict; the logged G loss gains the reference's
VGG feature term) with --perceptual (that term trains the generator) and --vgg_loss_weight W (its weight, default 6e-3)
and --resume [PATH] (continue training from the training-state file a run writes beside its checkpoints at every
--save_epochs boundary and at its end; without PATH this run's own <save_dir>/model/<model_name>_train_state.pkl) and
--ema_decay D (the optimizer kernel also keeps an exponential moving average of the weights, saved beside every
checkpoint as ..._ema.pkl; D in [0, 1), default 0: none; not DRCN) with --use_ema (--test_only / --test_single load it)
and --degrade (train on LR = (HR * k) shrunk + n instead of the clean bicubic shrink: a random anisotropic Gaussian blur and
Gaussian noise on the device, data.Degradation) with --blur_sigma LO,HI, --blur_prob P and --noise_sigma LO,HI, and
--degrade_test S1,S2,THETA_DEG,NOISE (the test sets under one fixed degradation); image folders only, not --synthetic;
and --jpeg_quality LO,HI (with --degrade: the degraded LR patch is also JPEG-compressed at a quality drawn from LO..HI and
decoded again, on the device, byte for byte as Pillow would) with --jpeg_prob P and --jpeg_subsampling {420,444}, and
--jpeg_test Q (every test image's LR input compressed at quality Q, behind --degrade_test where that is given).
--model_name RCAN (not in the reference: EDSR's trunk with channel attention, models.RCANNet) with --rcan_groups G,
--rcan_blocks B and --rcan_reduction R (defaults 10, 20, 16); every flag of the common trainer works with it but --tile.
--lpips_vgg PATH --lpips_lin PATH (a torchvision vgg16 state_dict and the `lpips` package's vgg.pth; both or neither):
test() also reports LPIPS (ops.lpips, on the device) beside PSNR and SSIM; with them --lpips_weight W adds W * LPIPS to the
training loss of every model but SRGAN and DRCN.  RGB only (--num_channels 3).
--model_name RDN (not in the reference: residual dense blocks on concat-free slice convolutions, models.RDNNet) with
--rdn_blocks D, --rdn_layers C and --rdn_growth G (defaults 16, 8, 64: the paper's net); every flag of the common trainer
works with it, --tile included.
--model_name SwinIR (not in the reference: shifted-window attention, models.SwinIRNet) with --swinir_dim, --swinir_depths,
--swinir_heads, --swinir_window, --swinir_mlp_ratio and --swinir_upsampler {pixelshuffle,pixelshuffledirect} (defaults: the
classical net, 180 channels, 6 x 6 layers, 6 heads, window 8, ratio 2); every flag of the common trainer but --tile.
--model_name ESRGAN (not in the reference: the RRDB generator, models.RRDBNet, on SRGAN's two-phase trainer) with
--rrdb_blocks NB and --rrdb_growth GC (defaults 23, 32), --pixel_weight, --vgg_loss_weight (default 1.0 for this model) and
--gan_weight (defaults 1e-2, 5e-3): --epoch_pretrain epochs of L1, then the adversarial phase on the relativistic average
GAN loss, which needs --vgg_weights PATH (conv5_4 features before the ReLU).  x4, RGB, one GPU; no --tile, --ssim_weight,
--fft_weight or --lpips_weight.  --net_interp A (with --test_only / --test_single) evaluates the blend
(1 - A) * pre-trained + A * adversarial generator, 0 <= A <= 1.
--discriminator {vgg,unet} (ESRGAN; default vgg): unet trains against Real-ESRGAN's U-Net discriminator with spectral
normalisation (models.UNetDiscriminatorSN, --unet_feat F channels, default 64; one logit a pixel, so any --crop_size that is
a multiple of 8) on --gan_type vanilla (ops.gan_logit_loss; the default with unet, where ragan is refused; ragan stays the
default with vgg).  Data parallelism is not part of it.
--vgg_layers SPEC (ESRGAN, with --vgg_weights): Real-ESRGAN's multi-layer VGG feature term in place of the conv5_4 one, an
L1 on VGG19 maps taken before their ReLUs: SPEC is name:weight,... (conv1_1 .. conv5_4) or `realesrgan`
(conv1_2:0.1,conv2_2:0.1,conv3_4:1,conv4_4:1,conv5_4:1); each tapped layer is one fused kernel (ops.vgg_feature_loss).
--degrade2 [SETTINGS.json] (train on Real-ESRGAN's second-order degradation, data.Degradation2: blur, resize, Gaussian or
Poisson noise and JPEG, twice, then a sinc filter, every stage a kernel on 8-bit patches; the file holds only overrides of
Degradation2's keywords), --usm (the training target and the degradation's input are the patches sharpened by
Real-ESRGAN's USMSharp; also with --degrade or alone) and --degrade2_test SEED (every test image under its own seeded chain);
image folders only; not with --degrade or --jpeg_quality.
--niqe_params PATH (an .npz with mu_pris_param and cov_pris_param): test() also reports NIQE (ops.niqe, on the device; no
ground truth) of the net's 8-bit output -- ' NIQE %.4f' on the --test_only line, a second line after --test_single.
--niqe_fit DIR --niqe_params OUT fits such a file from the pictures of DIR and exits.
--test_video IN [--video_out OUT] [--video_batch N] (load the checkpoint, super-resolve the YUV4MPEG2 stream IN -- 8-bit
4:2:0, 4:4:4 or mono; - = stdin -- in batches of N frames from file bytes to file bytes on the device, write OUT, default
<save_dir>/test_result/SR_result.y4m, - = stdout; honours --tile and --self_ensemble; no training).
--model_name VESPCN (not in the reference: ESPCN's video follow-up, models.VESPCNNet): three consecutive LR frames, the two
neighbours warped onto the centre one by a learned coarse-to-fine flow (fused HIP: ops.motion_fuse), ESPCN's trunk on the
nine (three for Y) channels; loss MSE + --mc_weight W * motion-compensation MSE + --flow_weight W * flow smoothness
(defaults 0.01 and 0.001), --vespcn_max_flow PX (default 8).  Training reads clip folders, data_dir/<dataset>/<clip>/<frames>
(data.ClipDataset), or --synthetic; --crop_size / --scale_factor must be a multiple of 4.  --test_single and test() on
single pictures use the picture as its own neighbours.  One GPU; no --tile, --self_ensemble, --degrade*, --usm, --jpeg_*,
--ssim_weight, --fft_weight, --lpips_weight.  --test_video computes frame t from frames t-1, t, t+1 of the stream (the ends
use themselves; as many frames out as in); test() on a test set of clip folders evaluates every frame with its neighbours.
Which flags go with which model and with each other is said once, by the trainer class (sr_trainers: trainer_class(model_name).
check_flags(args), a ValueError naming the flag); parse_args reports it as a usage error and itself holds only the rules
about the run: the modes --niqe_fit / --test_video / --test_only / --test_single against each other and --resume, files
that must exist, ESRGAN's --vgg_weights when it trains.
Multi-GPU: python -m torch.distributed.run --nproc-per-node N main.py ..."""
import argparse
import os

# data.Degradation2's keywords (tests hold the two lists together): what --degrade2's SETTINGS.json may override
DEGRADE2_KEYS = ('kernel_sizes', 'kernel_sizes2', 'kernel_prob', 'kernel_prob2', 'sinc_prob', 'sinc_prob2', 'blur_sigma',
                 'blur_sigma2', 'betag_range', 'betag_range2', 'betap_range', 'betap_range2', 'second_blur_prob',
                 'resize_prob', 'resize_prob2', 'resize_range', 'resize_range2', 'gaussian_noise_prob',
                 'gaussian_noise_prob2', 'noise_range', 'noise_range2', 'poisson_scale_range', 'poisson_scale_range2',
                 'gray_noise_prob', 'gray_noise_prob2', 'jpeg_range', 'jpeg_range2', 'final_sinc_prob', 'jpeg_subsampling')


def _names(text):
    """--train_dataset / --test_dataset: the reference declares them `type=list` (main.py:18-19), which turns a value
    given on the command line into its characters ('DIV2K' -> ['D','I','V','2','K']); here a value is one name or a
    comma-separated list of names."""
    return [n for n in (t.strip() for t in str(text).split(',')) if n]


def _tile(text):
    """--tile: a positive number of net-input pixels, or 'auto'."""
    if str(text).lower() == 'auto':
        return 'auto'
    v = int(text)
    if v < 1:
        raise argparse.ArgumentTypeError("--tile takes a positive integer or 'auto'")
    return v


def _positive(text):
    """--rcan_groups / --rcan_blocks / --rcan_reduction: a whole number >= 1."""
    try:
        v = int(text)
    except ValueError:
        v = 0
    if v < 1:
        raise argparse.ArgumentTypeError("a whole number >= 1 is expected, got %r" % (text,))
    return v


def _depths(text):
    """--swinir_depths: layers per RSTB, whole numbers >= 1, comma-separated."""
    try:
        v = tuple(int(t) for t in text.split(','))
    except ValueError:
        v = ()
    if not v or min(v) < 1:
        raise argparse.ArgumentTypeError("whole numbers >= 1, comma-separated, are expected, got %r" % (text,))
    return v


def _mlp_ratio(text):
    """--swinir_mlp_ratio: a number > 0."""
    try:
        v = float(text)
    except ValueError:
        v = 0.0
    if not v > 0:
        raise argparse.ArgumentTypeError("a number > 0 is expected, got %r" % (text,))
    return v


def _unit_interval(text):
    """--ssim_weight: a number in [0, 1] (NaN fails both comparisons)."""
    try:
        v = float(text)
    except ValueError:
        v = float('nan')
    if not 0.0 <= v <= 1.0:
        raise argparse.ArgumentTypeError("--ssim_weight takes a number in [0, 1], got %r" % (text,))
    return v


def _fft_weight(text):
    """--fft_weight: a finite number >= 0."""
    try:
        v = float(text)
    except ValueError:
        v = float('nan')
    if not 0.0 <= v < float('inf'):
        raise argparse.ArgumentTypeError("--fft_weight takes a number >= 0, got %r" % (text,))
    return v


def _loss_weight(text):
    """--gan_weight / --pixel_weight: a finite number >= 0."""
    try:
        v = float(text)
    except ValueError:
        v = float('nan')
    if not 0.0 <= v < float('inf'):
        raise argparse.ArgumentTypeError("a number >= 0 is expected, got %r" % (text,))
    return v


def _floats(text, n, flag):
    try:
        v = tuple(float(s) for s in str(text).split(','))
    except ValueError:
        v = ()
    if len(v) != n or not all(x == x and abs(x) != float('inf') for x in v):
        raise argparse.ArgumentTypeError("%s takes %d comma-separated numbers, got %r" % (flag, n, text))
    return v


def _blur_sigma(text):
    """--blur_sigma LO,HI: 0 < LO <= HI, in pixels."""
    lo, hi = _floats(text, 2, '--blur_sigma')
    if not 0.0 < lo <= hi:
        raise argparse.ArgumentTypeError("--blur_sigma takes LO,HI with 0 < LO <= HI, got %r" % (text,))
    return lo, hi


def _noise_sigma(text):
    """--noise_sigma LO,HI: 0 <= LO <= HI, in 8-bit levels."""
    lo, hi = _floats(text, 2, '--noise_sigma')
    if not 0.0 <= lo <= hi:
        raise argparse.ArgumentTypeError("--noise_sigma takes LO,HI with 0 <= LO <= HI, got %r" % (text,))
    return lo, hi


def _blur_prob(text):
    """--blur_prob: a number in [0, 1] (NaN fails both comparisons)."""
    try:
        v = float(text)
    except ValueError:
        v = float('nan')
    if not 0.0 <= v <= 1.0:
        raise argparse.ArgumentTypeError("--blur_prob takes a number in [0, 1], got %r" % (text,))
    return v


def _degrade_test(text):
    """--degrade_test S1,S2,THETA_DEG,NOISE: S1, S2 > 0 pixels, the angle in degrees, NOISE >= 0 8-bit levels."""
    s1, s2, th, ns = _floats(text, 4, '--degrade_test')
    if not (s1 > 0 and s2 > 0 and ns >= 0):
        raise argparse.ArgumentTypeError("--degrade_test takes S1,S2,THETA_DEG,NOISE with S1, S2 > 0 and NOISE >= 0, got %r"
                                         % (text,))
    return s1, s2, th, ns


def _degrade2_settings(path):
    """--degrade2 SETTINGS.json: a JSON object of data.Degradation2 keyword overrides; unknown keys are named."""
    import json
    try:
        with open(path) as f:
            settings = json.load(f)
    except (OSError, ValueError) as e:
        raise argparse.ArgumentTypeError("--degrade2: cannot read %r (%s)" % (path, e))
    if not isinstance(settings, dict):
        raise argparse.ArgumentTypeError("--degrade2: %r must hold a JSON object of Degradation2 settings" % (path,))
    unknown = sorted(set(settings) - set(DEGRADE2_KEYS))
    if unknown:
        raise argparse.ArgumentTypeError("--degrade2: %r holds unknown key%s %s (known: %s)"
                                         % (path, "s" if len(unknown) > 1 else "", ", ".join(unknown), ", ".join(DEGRADE2_KEYS)))
    return settings


def _jpeg_int(text, flag):
    try:
        v = int(str(text).strip())
    except ValueError:
        v = 0
    if not 1 <= v <= 100:
        raise argparse.ArgumentTypeError("%s takes whole numbers in 1..100, got %r" % (flag, text))
    return v


def _jpeg_quality(text):
    """--jpeg_quality LO,HI: whole numbers, 1 <= LO <= HI <= 100."""
    parts = str(text).split(',')
    if len(parts) != 2:
        raise argparse.ArgumentTypeError("--jpeg_quality takes LO,HI, got %r" % (text,))
    lo, hi = (_jpeg_int(t, '--jpeg_quality') for t in parts)
    if lo > hi:
        raise argparse.ArgumentTypeError("--jpeg_quality takes LO,HI with LO <= HI, got %r" % (text,))
    return lo, hi


def _jpeg_test(text):
    """--jpeg_test Q: a whole number in 1..100."""
    return _jpeg_int(text, '--jpeg_test')


def _jpeg_prob(text):
    """--jpeg_prob: a number in [0, 1] (NaN fails both comparisons)."""
    try:
        v = float(text)
    except ValueError:
        v = float('nan')
    if not 0.0 <= v <= 1.0:
        raise argparse.ArgumentTypeError("--jpeg_prob takes a number in [0, 1], got %r" % (text,))
    return v


def parse_args(argv=None):
    from pytorch_super_resolution_model_collection_amd.sr_trainers import model_names, trainer_class
    p = argparse.ArgumentParser(description="MI355X-native SR collection (reference-compatible CLI)")
    p.add_argument('--model_name', type=str, default='SRGAN',
                   choices=model_names(), help='The type of model')
    p.add_argument('--data_dir', type=str, default='../Data')
    p.add_argument('--train_dataset', type=_names, default=['DIV2K'], help='The name(s) of the training dataset, comma-separated')
    p.add_argument('--test_dataset', type=_names, default=['Set5', 'Set14', 'Urban100'], help='The name(s) of the test dataset, comma-separated')
    p.add_argument('--crop_size', type=int, default=128, help='Size of cropped HR image')
    p.add_argument('--num_threads', type=int, default=4, help='number of threads for data loader to use')
    p.add_argument('--num_channels', type=int, default=3, help='The number of channels to super-resolve')
    p.add_argument('--scale_factor', type=int, default=4, help='Size of scale factor')
    p.add_argument('--num_epochs', type=int, default=100, help='The number of epochs to run')
    p.add_argument('--save_epochs', type=int, default=10, help='Save trained model every this epochs')
    p.add_argument('--batch_size', type=int, default=16, help='training batch size')
    p.add_argument('--test_batch_size', type=int, default=1, help='testing batch size')
    p.add_argument('--save_dir', type=str, default='Result_DIV2K', help='Directory name to save the results')
    p.add_argument('--lr', type=float, default=0.00001)
    p.add_argument('--gpu_mode', type=bool, default=True)
    p.add_argument('--synthetic', action='store_true',
                   help='train / test on seeded random patches instead of the image folders under --data_dir '
                        '(without it a missing folder is an error, as in the reference)')
    p.add_argument('--steps_per_epoch', type=int, default=8, help='--synthetic: batches per epoch')
    p.add_argument('--epoch_pretrain', type=int, default=50, help='SRGAN generator pre-training epochs (srgan.py:179)')
    p.add_argument('--precision', type=str, default='mixed', choices=['mixed', 'bf16x3', 'bf16x6', 'fp32'])
    p.add_argument('--eager', action='store_true', help='launch every kernel of a train step from Python (default: replay the step as a hipGraph)')
    p.add_argument('--sync_bn', action='store_true',
                   help='data-parallel SRGAN: BatchNorm statistics over the GLOBAL batch (all-reduce of the [2C] sums per '
                        'BatchNorm call; default: per-shard statistics), i.e. the single-process step of the reference')
    p.add_argument('--prune_dead_grads', action='store_true',
                   help='SRGAN: skip the two gradient computations of the reference iteration that nothing reads '
                        '(G gradients of the D step, D parameter gradients of the G step); same parameters after every step')
    p.add_argument('--test_single', type=str, default=None, metavar='PATH',
                   help='no training: load the checkpoint, super-resolve this picture file (the Y channel with '
                        '--num_channels 1, colour restored from the bicubic Cb / Cr) and print the name of the PNG written')
    p.add_argument('--test_video', type=str, default=None, metavar='IN',
                   help='no training: load the checkpoint and super-resolve this YUV4MPEG2 stream (.y4m: 8-bit 4:2:0, 4:4:4 '
                        'or mono, progressive; - = stdin, e.g. from ffmpeg -f yuv4mpegpipe) in batches on the device; '
                        'honours --tile and --self_ensemble')
    p.add_argument('--video_out', type=str, default=None, metavar='OUT',
                   help='--test_video: where the super-resolved stream goes (- = stdout); default: '
                        '<save_dir>/test_result/SR_result.y4m')
    p.add_argument('--video_batch', type=int, default=8, metavar='N',
                   help='--test_video: frames per batch (default 8)')
    p.add_argument('--save_test_images', action='store_true',
                   help='test(): write every result image to <save_dir>/test_result/<dataset>/ and report the bicubic PSNR')
    p.add_argument('--tile', type=_tile, default=None, metavar='N|auto',
                   help='--test_single and test(): cut the picture into overlapping tiles of N x N net-input pixels, run '
                        'them as batches and stitch the exact result (auto: only pictures too large for one pass); '
                        'default: one pass')
    p.add_argument('--test_only', action='store_true',
                   help='no training: load the checkpoint, run test() on the test sets (honours --save_test_images and '
                        '--tile) and print PSNR and SSIM per dataset')
    p.add_argument('--eval_domain', type=str, default=None, choices=['float', 'u8', 'y8'],
                   help='test(): also report PSNR and SSIM in this domain -- float: the tensors as they are; u8: the 8-bit '
                        'picture that --save_test_images writes; y8: the luma of that picture')
    p.add_argument('--eval_shave', type=int, default=None, metavar='N',
                   help='test(): leave a border of N pixels out of the --eval_domain numbers (tables use the scale factor)')
    p.add_argument('--self_ensemble', action='store_true',
                   help='--test_single and test(): the x8 geometric self-ensemble ("EDSR+"): the net on the eight flips / '
                        'rotations of the picture, each result transformed back, the eight averaged; works with --tile')
    p.add_argument('--ssim_weight', type=_unit_interval, default=0.0, metavar='A',
                   help='train on (1 - A) * the pixel loss of the model + A * (1 - SSIM) (ops.ssim_loss; LapSRN: both '
                        'levels); A in [0, 1], default 0: the pixel loss alone, as the reference.  Not for SRGAN and DRCN')
    p.add_argument('--fft_weight', type=_fft_weight, default=0.0, metavar='W',
                   help='add W * the L1 on the full 2-D Fourier spectrum of prediction - target (ops.fft_loss, BasicSR\'s '
                        'FFTLoss; LapSRN: both levels) to the training loss; W >= 0, default 0: none.  HR patches of at '
                        'most 256 on a side.  Not for SRGAN and DRCN')
    p.add_argument('--fft_norm', choices=('backward', 'ortho'), default='backward',
                   help='--fft_weight: the transform unscaled ("backward", torch.fft.fft2\'s default) or divided by '
                        'sqrt(H W) ("ortho")')
    p.add_argument('--vgg_weights', type=str, default=None, metavar='PATH',
                   help='SRGAN: a torchvision vgg19 state_dict file; the G loss then includes the VGG feature term of the '
                        'reference, 6e-3 * MSE of vgg19.features[:9] -- logged only, as there, unless --perceptual')
    p.add_argument('--perceptual', action='store_true',
                   help='SRGAN: the VGG feature term trains the generator (ops.perceptual_loss; the reference detaches it). '
                        'Needs --vgg_weights and --num_channels 3')
    p.add_argument('--vgg_loss_weight', type=float, default=None, metavar='W',
                   help='SRGAN: weight of the VGG feature term in the G loss (default 6e-3, srgan.py:306); W >= 0.  '
                        'ESRGAN: default 1.0')
    p.add_argument('--resume', type=str, nargs='?', const='auto', default=None, metavar='PATH',
                   help='continue training from a training-state file (weights, optimizer state, learning rates, epoch, '
                        'loss history, random generators): PATH, or without one the file this run writes, '
                        '<save_dir>/model/<model_name>_train_state.pkl.  Runs continue at epoch boundaries only')
    p.add_argument('--ema_decay', type=float, default=0.0, metavar='D',
                   help='keep an exponential moving average of the weights, ema += (1 - D) * (w - ema) after every step, '
                        'inside the optimizer kernel; written beside every checkpoint as ..._ema.pkl.  D in [0, 1), '
                        'default 0: none.  Not for DRCN')
    p.add_argument('--use_ema', action='store_true',
                   help='--test_only / --test_single: load the EMA weights (..._ema.pkl) instead of the plain checkpoint')
    p.add_argument('--degrade', action='store_true',
                   help='train on the degradation model LR = (HR * k) shrunk + n instead of the clean bicubic shrink: per '
                        'patch a random anisotropic Gaussian blur in front of the shrink and Gaussian noise behind it, on '
                        'the device (data.Degradation).  Image folders only')
    p.add_argument('--blur_sigma', type=_blur_sigma, default=(0.2, 4.0), metavar='LO,HI',
                   help='--degrade: range of the blur\'s two standard deviations in HR pixels (default 0.2,4.0)')
    p.add_argument('--blur_prob', type=_blur_prob, default=1.0, metavar='P',
                   help='--degrade: probability that a patch is blurred at all (default 1)')
    p.add_argument('--noise_sigma', type=_noise_sigma, default=(0.0, 10.0), metavar='LO,HI',
                   help='--degrade: range of the noise\'s standard deviation in 8-bit levels (default 0,10; 0,0: none)')
    p.add_argument('--degrade_test', type=_degrade_test, default=None, metavar='S1,S2,THETA_DEG,NOISE',
                   help='test(): every test image under this one degradation (blur standard deviations, angle in degrees, '
                        'noise standard deviation; the noise seeded by the image\'s index).  Image folders only')
    p.add_argument('--degrade2', type=_degrade2_settings, nargs='?', const={}, default=None, metavar='SETTINGS.json',
                   help='train on Real-ESRGAN\'s second-order degradation (blur, resize, noise, JPEG, twice, then a sinc '
                        'filter), on the device; SETTINGS.json holds only overrides of data.Degradation2\'s keywords.  Image '
                        'folders only')
    p.add_argument('--usm', action='store_true',
                   help='sharpen the 8-bit training patches with Real-ESRGAN\'s USMSharp first: the target and the input of '
                        'the shrink or the degradation are the sharpened patches.  Image folders only')
    p.add_argument('--degrade2_test', type=int, default=None, metavar='SEED',
                   help='degrade every test image by its own chain of --degrade2\'s settings, drawn from a private generator '
                        'seeded by (SEED, index): an item is the same on every read.  Image folders only')
    p.add_argument('--jpeg_quality', type=_jpeg_quality, default=None, metavar='LO,HI',
                   help='--degrade: also JPEG-compress the degraded LR patch at a quality drawn from LO..HI (whole numbers '
                        'in 1..100) and decode it again, on the device (default: no JPEG stage)')
    p.add_argument('--jpeg_prob', type=_jpeg_prob, default=1.0, metavar='P',
                   help='--jpeg_quality: probability that a patch is compressed at all (default 1)')
    p.add_argument('--jpeg_subsampling', type=str, default='420', choices=['420', '444'],
                   help='--jpeg_quality / --jpeg_test: chroma subsampling, 4:2:0 (Pillow\'s default) or 4:4:4')
    p.add_argument('--jpeg_test', type=_jpeg_test, default=None, metavar='Q',
                   help='test(): every test image\'s LR input JPEG-compressed at quality Q and decoded again, behind '
                        '--degrade_test where that is given.  Image folders only')
    p.add_argument('--rcan_groups', type=_positive, default=10, metavar='G', help='RCAN: residual groups (default 10)')
    p.add_argument('--rcan_blocks', type=_positive, default=20, metavar='B',
                   help='RCAN: residual channel attention blocks per group (default 20)')
    p.add_argument('--rcan_reduction', type=_positive, default=16, metavar='R',
                   help='RCAN: channel reduction of the attention gate, a divisor of 64 (default 16)')
    p.add_argument('--lpips_vgg', type=str, default=None, metavar='PATH',
                   help='a torchvision vgg16 state_dict file; with --lpips_lin, test() also reports LPIPS (Zhang et al. '
                        '2018, the VGG variant; ops.lpips) beside PSNR and SSIM.  Needs --num_channels 3')
    p.add_argument('--lpips_lin', type=str, default=None, metavar='PATH',
                   help='the linear layers of LPIPS: the `lpips` package\'s vgg.pth (lin{l}.model.1.weight); goes with '
                        '--lpips_vgg')
    p.add_argument('--lpips_weight', type=float, default=0.0, metavar='W',
                   help='add W * LPIPS(prediction, target) to the training loss (LapSRN: both levels); W >= 0, default 0: '
                        'none.  Needs --lpips_vgg and --lpips_lin; HR patches of at least 16 on a side (LapSRN: 32).  Not '
                        'for SRGAN and DRCN')
    p.add_argument('--rdn_blocks', type=_positive, default=16, metavar='D', help='RDN: residual dense blocks (default 16)')
    p.add_argument('--rdn_layers', type=_positive, default=8, metavar='C',
                   help='RDN: convolutions per residual dense block (default 8)')
    p.add_argument('--rdn_growth', type=_positive, default=64, metavar='G',
                   help='RDN: growth rate, channels every layer adds: 16, 32, 48 or 64 (default 64)')
    p.add_argument('--swinir_dim', type=_positive, default=180, metavar='C', help='SwinIR: embedding channels (default 180)')
    p.add_argument('--swinir_depths', type=_depths, default=(6, 6, 6, 6, 6, 6), metavar='D1,D2,...',
                   help='SwinIR: layers of every residual Swin Transformer block (default 6,6,6,6,6,6)')
    p.add_argument('--swinir_heads', type=_positive, default=6, metavar='H', help='SwinIR: attention heads (default 6)')
    p.add_argument('--swinir_window', type=_positive, default=8, metavar='W', help='SwinIR: window size, 2 .. 8 (default 8)')
    p.add_argument('--swinir_mlp_ratio', type=_mlp_ratio, default=2.0, metavar='R',
                   help='SwinIR: hidden channels of the MLP over the embedding channels (default 2)')
    p.add_argument('--swinir_upsampler', type=str, default='pixelshuffle', choices=['pixelshuffle', 'pixelshuffledirect'],
                   help='SwinIR: the classical (pixelshuffle) or the lightweight (pixelshuffledirect) reconstruction')
    p.add_argument('--rrdb_blocks', type=_positive, default=23, metavar='NB',
                   help='ESRGAN: residual-in-residual dense blocks of the generator (default 23)')
    p.add_argument('--rrdb_growth', type=_positive, default=32, metavar='GC',
                   help='ESRGAN: growth channels of the dense blocks: 16, 32, 48 or 64 (default 32)')
    p.add_argument('--gan_weight', type=_loss_weight, default=5e-3, metavar='W',
                   help='ESRGAN: weight of the relativistic average GAN term in the G loss (default 5e-3)')
    p.add_argument('--pixel_weight', type=_loss_weight, default=1e-2, metavar='W',
                   help='ESRGAN: weight of the L1 pixel term in the G loss of the adversarial phase (default 1e-2)')
    p.add_argument('--net_interp', type=float, default=None, metavar='A',
                   help='ESRGAN, with --test_only / --test_single: evaluate (1 - A) * the pre-trained generator + A * the '
                        'adversarially trained one (network interpolation of the ESRGAN paper); A in [0, 1]')
    p.add_argument('--discriminator', type=str, default=None, choices=['vgg', 'unet'],
                   help='ESRGAN: the discriminator of the adversarial phase: vgg (default; SRGAN\'s body ending in a logit) '
                        'or unet (Real-ESRGAN\'s U-Net with spectral normalisation, one logit a pixel, any --crop_size that '
                        'is a multiple of 8)')
    p.add_argument('--gan_type', type=str, default=None, choices=['ragan', 'vanilla'],
                   help='ESRGAN: the GAN loss on the discriminator\'s logits: ragan (relativistic average; default with '
                        '--discriminator vgg) or vanilla (default with, and the only one for, --discriminator unet)')
    p.add_argument('--unet_feat', type=int, default=None, metavar='F',
                   help='ESRGAN with --discriminator unet: channels of the U-Net\'s first layer (default 64)')
    p.add_argument('--vgg_layers', type=str, default=None, metavar='SPEC',
                   help='ESRGAN: train on Real-ESRGAN\'s multi-layer VGG feature term instead of the single conv5_4 one: '
                        'name:weight,... over VGG19 conv layers taken before their ReLUs (conv1_1 .. conv5_4), or the word '
                        'realesrgan = conv1_2:0.1,conv2_2:0.1,conv3_4:1,conv4_4:1,conv5_4:1.  Needs --vgg_weights; the whole '
                        'term is weighed by --vgg_loss_weight')
    p.add_argument('--mc_weight', type=_loss_weight, default=None, metavar='W',
                   help='VESPCN: weight of the motion-compensation MSE of the warped neighbours (default 0.01: the paper\'s '
                        'value as remembered, unchecked)')
    p.add_argument('--flow_weight', type=_loss_weight, default=None, metavar='W',
                   help='VESPCN: weight of the flow-smoothness (Huber) term (default 0.001: the paper\'s value as '
                        'remembered, unchecked)')
    p.add_argument('--vespcn_max_flow', type=float, default=None, metavar='PX',
                   help='VESPCN: pixels one unit of the coarse flow\'s tanh stands for; the fine stage adds a quarter of it '
                        '(default 8; the paper gives no scale, this is the project\'s choice)')
    p.add_argument('--niqe_params', type=str, default=None, metavar='PATH',
                   help='NIQE\'s pristine model, an .npz with mu_pris_param [36] and cov_pris_param [36, 36] (BasicSR\'s '
                        'niqe_pris_params.npz, or one written by --niqe_fit): test() also reports NIQE (Mittal et al. 2013; '
                        'ops.niqe, on the device, no ground truth needed) of the net\'s 8-bit output, --eval_shave pixels off '
                        'each side; --test_only appends it to its line, --test_single prints it on a second line.  With '
                        '--niqe_fit: the file to write')
    p.add_argument('--niqe_fit', type=str, default=None, metavar='DIR',
                   help='fit NIQE\'s pristine model from the image files of DIR (blocks of 96 x 96 sharper than 0.75 of '
                        'each picture\'s sharpest), write it to --niqe_params OUT (which must not exist), print the number '
                        'of blocks used and exit.  Goes with no other mode flag')
    args = p.parse_args(argv)
    if args.test_video is not None:
        for flag in ('test_only', 'test_single', 'resume', 'save_test_images', 'niqe_fit'):
            if getattr(args, flag):
                p.error('--test_video super-resolves a stream and exits: it does not go with --%s' % flag)
        if args.test_video != '-' and not os.path.exists(args.test_video):   # a named pipe is a source too
            p.error('--test_video %s: no such file' % args.test_video)
        if args.video_batch <= 0:
            p.error('--video_batch must be positive (got %d)' % args.video_batch)
    elif args.video_out is not None:
        p.error('--video_out goes with --test_video IN')
    if args.niqe_fit is not None:
        if not args.niqe_params:
            p.error('--niqe_fit DIR needs --niqe_params OUT, the .npz file to write')
        for flag in ('test_only', 'test_single', 'resume', 'save_test_images'):
            if getattr(args, flag):
                p.error('--niqe_fit fits a parameter file and exits: it does not go with --%s' % flag)
        if not os.path.isdir(args.niqe_fit):
            p.error('--niqe_fit %s: no such directory' % args.niqe_fit)
        if os.path.exists(args.niqe_params):
            p.error('--niqe_params %s exists: --niqe_fit does not overwrite a parameter file' % args.niqe_params)
    elif args.niqe_params is not None and not os.path.isfile(args.niqe_params):
        p.error('--niqe_params %s: no such file' % args.niqe_params)
    if args.resume and args.test_only:
        p.error('--resume continues a training run; --test_only does not train')
    if args.net_interp is not None and not (args.test_only or args.test_single):
        p.error('--net_interp blends two finished checkpoints: it goes with --test_only or --test_single')
    # which flags go with the model and with each other: the trainer class says (sr_trainers: check_flags)
    trainer = trainer_class(args.model_name)
    try:
        trainer.check_flags(args)
    except (ValueError, NotImplementedError) as e:   # (NotImplementedError: a model without data parallelism)
        p.error(str(e))
    if args.model_name == 'ESRGAN' and not args.vgg_weights and not (args.test_only or args.test_single):
        p.error('--vgg_weights PATH is required: ESRGAN\'s adversarial phase trains on VGG19 conv5_4 features (a '
                'torchvision vgg19 state_dict file)')
    for flag, value in trainer.flag_defaults(args).items():
        setattr(args, flag, value)
    return check_args(args)


def check_args(args):   # main.py:39-57
    args.save_dir = os.path.join(args.save_dir, args.model_name)
    os.makedirs(args.save_dir, exist_ok=True)
    if args.num_epochs < 1:
        print('number of epochs must be larger than or equal to one')
    if args.batch_size < 1:
        print('batch size must be larger than or equal to one')
    return args


def report(net, args):
    """One line per dataset after test(), from the metric table test() fills (evaluation.report_lines): every number it
    stored.  Without --test_only, --save_test_images or --eval_domain / --eval_shave numbers nothing is printed."""
    from pytorch_super_resolution_model_collection_amd import evaluation
    for line in evaluation.report_lines(net, args.model_name, args.save_test_images, args.test_only or args.save_test_images):
        print(line)


def niqe_fit(args):
    """--niqe_fit DIR --niqe_params OUT: NIQE's own fit (utils.fit_niqe_params) over the image files of DIR."""
    import torch
    from pytorch_super_resolution_model_collection_amd import data, utils
    names = sorted(f for f in os.listdir(args.niqe_fit) if data.is_image_file(f))
    if not names:
        raise SystemExit('--niqe_fit %s: no image files' % args.niqe_fit)
    pictures = (torch.tensor(data.load_img(os.path.join(args.niqe_fit, f))).permute(2, 0, 1) for f in names)
    mu_p, cov_p, rows = utils.fit_niqe_params(pictures)
    utils.save_niqe_params(args.niqe_params, mu_p, cov_p)
    print('NIQE parameters fitted from %d blocks of %d pictures: %s' % (rows, len(names), args.niqe_params))


def main(argv=None):
    args = parse_args(argv)
    if args is None:
        exit()
    if args.test_video and args.video_out == '-':   # stdout carries the stream and nothing else: messages go to stderr
        import contextlib
        import sys
        sink = sys.stdout.buffer
        with contextlib.redirect_stdout(sys.stderr):
            return run(args, sink)
    return run(args)


def run(args, video_sink=None):
    import __graft_entry__
    __graft_entry__.build()
    import pytorch_super_resolution_model_collection_amd as pkg
    if args.niqe_fit is not None:
        return niqe_fit(args)
    from pytorch_super_resolution_model_collection_amd.sr_trainers import model_names, trainer_class
    pkg.ops.set_precision(args.precision)
    net = trainer_class(args.model_name)(args)   # main.py:70-89
    if args.test_single:                     # main.py:102: net.test_single(img_fn)
        print(net.test_single(args.test_single))
        if args.niqe_params:
            print('NIQE %.4f' % net.test_single_niqe)
        return net
    if args.test_video:
        net.test_video(args.test_video, video_sink if video_sink is not None else args.video_out, args.video_batch)
        return net
    if not args.test_only:
        net.train()                          # main.py:96
    net.test(save_images=True) if args.save_test_images else net.test()   # main.py:99
    report(net, args)
    return net


if __name__ == '__main__':
    main()
