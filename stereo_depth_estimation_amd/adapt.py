"""Fine-tune a checkpoint on rectified stereo pairs without labels (no counterpart in the reference).

    python -m stereo_depth_estimation_amd.adapt --checkpoint best.pt \\
        (--left-dir DIR --right-dir DIR | --dataset-root DIR) --output-dir DIR \\
        [--height H --width W] [--epochs 1] [--batch-size 16] [--lr 1e-5] [--weight-decay 0] [--precision fp32|bf16] \\
        [--w-smooth 0.1] [--edge-gamma 10] [--occ-tol 0.5] [--no-uncertainty] [--max-samples 0] [--seed 42] \\
        [--base-channels 32] [--read-threads 16] [--device cuda] [--ssim-weight 0] \\
        [--proxy-weight 0] [--proxy-only] [--proxy-num-disparities 64] [--proxy-block-size 5] [--proxy-mode 3way] \\
        [--proxy-cost bt|census] [--proxy-census-window 7x9] [--eval-uncertainty]

Runs ``selfsup.adapt_epoch`` over the pairs: the photometric + smoothness objective of ``sd_selfsup_loss`` (selfsup.py,
INTEGRATION.md "sd_selfsup_loss") through the model's training forward, the hand-scheduled backward and AdamW. The frames
are taken as rectified: FoundationStereo's are, for a pair of directories that is the user's statement. Frames are paired
and batched as the predict tool does (``pair_by_stem`` / ``discover_samples``, ``plan_batches``, the native PNG reader
into pinned memory, ``sd_stereo_preprocess`` with the left frame standing in for the label).

Writes ``<output-dir>/adapted.pt``, a checkpoint in ``cli.save_checkpoint``'s format (what the live app, ``predict`` and
the trainer's ``--resume`` read), and ``<output-dir>/adapt_meta.json``, also printed as one JSON line: the arguments, per
epoch ``loss``, ``photo``, ``smooth`` and ``visible_fraction``, and the photometric loss of the first and the last epoch.
With ``--dataset-root`` the labels are not used for training; they measure it: the EPE over the samples (``sd_disp_export``'s
metric rows, as ``predict`` evaluates) is recorded before and after. ``--device cpu`` is rejected (no CPU path).

``--ssim-weight A`` (0..1, default 0) mixes the SSIM dissimilarity of a 3 x 3 window into the photometric error,
``(1 - A) e + A s`` (``SelfSupLoss(ssim=A)``, ``sd_selfsup_loss_ssim``): for rigs whose two sensors differ in gain or
exposure. 0.85 is the literature's mix, not an optimum measured here. With A > 0 the epochs also carry ``ssim``, the mean
s over the counted pixels, and the meta ``ssim_first`` / ``ssim_last``.

``--proxy-weight W`` (default 0: off) adds proxy supervision (proxy.py, INTEGRATION.md "sd_proxy_loss"): the device
semi-global matcher labels the pixels it is sure of on every batch, and the heads are trained on those labels in the
reference's NLL form beside the photometric term, with weight W. ``--proxy-only`` trains on the labels alone (no check
stage, no photometric stage). ``--proxy-num-disparities`` (64), ``--proxy-block-size`` (5) and ``--proxy-mode`` (3way)
are the matcher's; they are parameters, not measured optima. The batch size is then at most 64 (the matcher's streams)
and the width must exceed the disparity range. With W > 0 the meta gains the proxy arguments, the epochs ``proxy_loss``,
``proxy_mae`` and ``proxy_fraction``, and the meta ``proxy_mae_first`` / ``proxy_mae_last``.

``--proxy-cost census`` labels with the census / Hamming pixel cost in place of Birchfield-Tomasi (``StereoSGM(cost=
"census")``, INTEGRATION.md "The census cost"): it compares the order of the intensities inside each image, not the
intensities of the two cameras, so the labels do not move under a gain, exposure or gamma difference between the sensors,
the case the adaptation is for. ``--proxy-census-window HxW`` (rows x columns: 3x3, 5x5, 7x7 or 7x9, default 7x9) is its
window; both are parameters, not measured optima, and need a positive ``--proxy-weight``. The default stays ``bt``; with
``census`` the meta also carries ``proxy_cost`` and ``proxy_census_window``.

``--eval-uncertainty`` (needs ``--dataset-root``) also measures the log-variance head before and after, since the
adaptation losses push on it: ``sd_uncert_eval`` on the same maps (uncert.py, INTEGRATION.md "Uncertainty evaluation"),
20 cuts. The meta gains ``eval_uncertainty`` and ``uncertainty_before`` / ``uncertainty_after`` (``uncert.aggregate_rows``:
NLL, coverage, AUSE, AURG, the sparsification curves); without the flag it is what it was.
"""

from __future__ import annotations

import argparse
import json
import time
from pathlib import Path

import numpy as np
import torch

from . import _lib as L
from .check import check_params
from .proxy import MAX_STREAMS as PROXY_MAX_BATCH, check_width, proxy_param
from .selfsup import SelfSupLoss, adapt_epoch, selfsup_params, ssim_param

META_KEYS = ("loss", "photo", "smooth", "visible_fraction")
PROXY_META_KEYS = ("proxy_loss", "proxy_mae", "proxy_fraction")
PROXY_DEFAULTS = dict(proxy_num_disparities=64, proxy_block_size=5, proxy_mode="3way", proxy_cost="bt")


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Fine-tune a checkpoint on rectified stereo pairs without labels.")
    p.add_argument("--checkpoint", type=str, required=True, help="Checkpoint of the training CLI (or the reference's).")
    p.add_argument("--left-dir", type=str, default=None, help="Directory of rectified left frames (paired by stem).")
    p.add_argument("--right-dir", type=str, default=None, help="Directory of rectified right frames.")
    p.add_argument("--dataset-root", type=str, default=None,
                   help="FoundationStereo tree: its labels are not trained on, they measure the EPE before and after.")
    p.add_argument("--output-dir", type=str, required=True, help="Where adapted.pt and adapt_meta.json go.")
    p.add_argument("--height", type=int, default=None, help="Model height (default: the checkpoint's).")
    p.add_argument("--width", type=int, default=None, help="Model width (default: the checkpoint's).")
    p.add_argument("--epochs", type=int, default=1)
    p.add_argument("--batch-size", type=int, default=16)
    p.add_argument("--lr", type=float, default=1e-5)
    p.add_argument("--weight-decay", type=float, default=0.0)
    p.add_argument("--precision", type=str, default="fp32", choices=("fp32", "bf16"))
    p.add_argument("--w-smooth", type=float, default=0.1, help="Weight of the smoothness term (a parameter, not an optimum).")
    p.add_argument("--edge-gamma", type=float, default=10.0, help="Edge sensitivity of the smoothness weights.")
    p.add_argument("--occ-tol", type=float, default=0.5, help="Occlusion tolerance of the visibility classes in pixels.")
    p.add_argument("--no-uncertainty", action="store_true", help="Plain photometric error, no log-variance weighting.")
    p.add_argument("--max-samples", type=int, default=0, help="Optional cap on number of samples.")
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--base-channels", type=int, default=32)
    p.add_argument("--read-threads", type=int, default=16, help="Host threads of the PNG reader.")
    p.add_argument("--device", type=str, default="cuda")
    p.add_argument("--ssim-weight", type=float, default=0.0,
                   help="Weight A in [0, 1] of the SSIM term in the photometric error, (1 - A) e + A s (0: none; 0.85 is "
                        "the literature's mix, not a measured optimum).")
    p.add_argument("--proxy-weight", type=float, default=0.0,
                   help="Weight of the proxy-label term: the device matcher's labels as a sparse target (0: off; a "
                        "parameter, not a measured optimum).")
    p.add_argument("--proxy-only", action="store_true", help="Train on the matcher's labels alone (needs --proxy-weight).")
    p.add_argument("--proxy-num-disparities", type=int, default=None,
                   help="Disparity range of the labelling matcher (default 64; a multiple of 16).")
    p.add_argument("--proxy-block-size", type=int, default=None, help="Block size of the labelling matcher (default 5).")
    p.add_argument("--proxy-mode", type=str, default=None, help="Path mode of the labelling matcher (default 3way).")
    p.add_argument("--proxy-cost", type=str, default=None, choices=("bt", "census"),
                   help="Pixel cost of the labelling matcher (default bt; census is invariant to monotone intensity maps).")
    p.add_argument("--proxy-census-window", type=str, default=None,
                   help="Census window HxW, rows x columns: 3x3, 5x5, 7x7 or 7x9 (default 7x9; needs --proxy-cost census).")
    p.add_argument("--eval-uncertainty", action="store_true",
                   help="Also evaluate the log-variance head before and after: sparsification, AUSE, coverage, NLL "
                        "(needs --dataset-root).")
    return p


def _resolve_device(device) -> torch.device:
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"--device {device}: the adapt tool runs only on a HIP device (no CPU path).")
    return dev


def adapt_options(left_dir=None, right_dir=None, dataset_root=None, output_dir=None, height=None, width=None,
                  epochs: int = 1, batch_size: int = 16, lr: float = 1e-5, weight_decay: float = 0.0,
                  precision: str = "fp32", w_smooth: float = 0.1, edge_gamma: float = 10.0, occ_tol: float = 0.5,
                  uncertainty: bool = True, max_samples: int = 0, seed: int = 42, base_channels: int = 32,
                  read_threads: int = 16, ssim_weight: float = 0.0, proxy_weight: float = 0.0, proxy_only: bool = False,
                  proxy_num_disparities=None, proxy_block_size=None, proxy_mode=None, proxy_cost=None,
                  proxy_census_window=None, eval_uncertainty: bool = False) -> dict:
    """The tool's options checked and gathered (raises ValueError), before a model or a device is touched. The proxy
    options are part of the result only with a positive ``proxy_weight``, ``proxy_cost`` and ``proxy_census_window``
    ("HxW") only when the cost is "census" (without them it is "bt"), ``eval_uncertainty`` only when it is set."""
    dirs = left_dir is not None or right_dir is not None
    if (dataset_root is not None) == dirs or (dirs and (left_dir is None or right_dir is None)):
        raise ValueError("give either --dataset-root or both --left-dir and --right-dir")
    if output_dir is None:
        raise ValueError("--output-dir is required.")
    if eval_uncertainty and dataset_root is None:
        raise ValueError("--eval-uncertainty needs --dataset-root (the ground truth it evaluates against).")
    if precision not in ("fp32", "bf16"):
        raise ValueError(f"--precision {precision}: adaptation trains, in fp32 or bf16 (fp8 is the inference-only forward).")
    if int(epochs) < 1:
        raise ValueError(f"--epochs must be >= 1, got: {epochs}")
    if int(batch_size) < 1:
        raise ValueError(f"--batch-size must be >= 1, got: {batch_size}")
    if not (np.isfinite(lr) and lr > 0):
        raise ValueError(f"--lr must be finite and > 0, got: {lr}")
    if not (np.isfinite(weight_decay) and weight_decay >= 0):
        raise ValueError(f"--weight-decay must be finite and >= 0, got: {weight_decay}")
    if int(max_samples) < 0:
        raise ValueError(f"--max-samples must be >= 0, got: {max_samples}")
    if (height is None) != (width is None):
        raise ValueError("--height and --width: give both or neither (default: the checkpoint's).")
    if height is not None and (height <= 0 or width <= 0 or height % 16 or width % 16):
        raise ValueError(f"--height / --width must be positive multiples of 16, got: {height} x {width}")
    try:
        _, w_smooth, _, _, edge_gamma = selfsup_params(w_smooth=w_smooth, gamma=edge_gamma)
        occ_tol, _ = check_params(occ_tol, float("inf"))
    except ValueError as e:
        raise ValueError(f"--w-smooth / --edge-gamma / --occ-tol: {e}") from None
    try:
        ssim_weight = ssim_param(ssim_weight)
    except ValueError as e:
        raise ValueError(f"--ssim-weight: {e}") from None
    proxy = _proxy_options(proxy_weight, proxy_only, proxy_num_disparities, proxy_block_size, proxy_mode, batch_size,
                           width, proxy_cost, proxy_census_window)
    return dict(left_dir=None if left_dir is None else str(left_dir), right_dir=None if right_dir is None else str(right_dir),
                dataset_root=None if dataset_root is None else str(dataset_root), output_dir=str(output_dir),
                height=height, width=width, epochs=int(epochs), batch_size=int(batch_size), lr=float(lr),
                weight_decay=float(weight_decay), precision=precision, w_smooth=w_smooth, edge_gamma=edge_gamma,
                occ_tol=occ_tol, uncertainty=bool(uncertainty), max_samples=int(max_samples), seed=int(seed),
                base_channels=int(base_channels), read_threads=int(read_threads), ssim_weight=ssim_weight, **proxy,
                **({"eval_uncertainty": True} if eval_uncertainty else {}))


def _proxy_options(weight, only, num_disparities, block_size, mode, batch_size, width, cost=None,
                   census_window=None) -> dict:
    """The proxy options checked: {} with the weight at 0 (no other proxy option may then be given)."""
    from .sgm import StereoSGM

    try:
        weight = proxy_param(weight)
    except ValueError as e:
        raise ValueError(f"--proxy-weight: {e}") from None
    given = dict(proxy_num_disparities=num_disparities, proxy_block_size=block_size, proxy_mode=mode, proxy_cost=cost,
                 proxy_census_window=census_window)
    if weight == 0:
        if only:
            raise ValueError("--proxy-only needs a positive --proxy-weight")
        extra = [f"--{k.replace('_', '-')}" for k, v in given.items() if v is not None]
        if extra:
            raise ValueError(f"{', '.join(extra)}: the matcher's options need a positive --proxy-weight")
        return {}
    out = {k: PROXY_DEFAULTS.get(k) if v is None else v for k, v in given.items()}
    try:
        m = StereoSGM(num_disparities=out["proxy_num_disparities"], block_size=out["proxy_block_size"],
                      mode=out["proxy_mode"], cost=out["proxy_cost"], census_window=out["proxy_census_window"])
    except (TypeError, ValueError) as e:
        raise ValueError(f"--proxy-num-disparities / --proxy-block-size / --proxy-mode / --proxy-cost / "
                         f"--proxy-census-window: {e}") from None
    if int(batch_size) > PROXY_MAX_BATCH:
        raise ValueError(f"--batch-size must be <= {PROXY_MAX_BATCH} with --proxy-weight (the matcher's streams), "
                         f"got: {batch_size}")
    if width is not None:
        try:
            check_width(width, m.min_disparity, m.num_disparities)
        except ValueError as e:
            raise ValueError(f"--width / --proxy-num-disparities: {e}") from None
    census = {} if m.cost == "bt" else dict(proxy_cost=m.cost, proxy_census_window="%dx%d" % m.census_window)
    return dict(proxy_weight=weight, proxy_only=bool(only), proxy_num_disparities=m.num_disparities,
                proxy_block_size=m.block_size, proxy_mode=m.mode, **census)


class _Frames:
    """The decode and the device copy of one batch: the native PNG reader into pinned memory (PIL for what it does not
    take), one set of buffers per source size, grown and never shrunk."""

    def __init__(self, device, bmax: int, has_gt: bool, threads: int):
        self.device, self.bmax, self.threads = device, bmax, threads
        self.kinds = ("left_rgb_path", "right_rgb_path") + (("disparity_path",) if has_gt else ())
        self._pin: dict = {}
        self._dev: dict = {}

    def load(self, hw, items) -> list[tuple]:
        """Parts (left, right[, ground truth]) of one source size each, uint8 [n, Hs, Ws, 3] on the device."""
        from .dataset import read_png_batch, read_rgb_uint8

        n = len(items)
        host = None
        if hw is not None:
            if hw not in self._pin:
                self._pin[hw] = tuple(torch.empty(self.bmax, *hw, 3, dtype=torch.uint8).pin_memory() for _ in self.kinds)
            views = tuple(t[:n] for t in self._pin[hw])
            # the pinned buffers are reused: the previous batch's copies must have left them
            torch.cuda.current_stream(self.device).synchronize()
            if all(read_png_batch([getattr(s, a) for s in items], hw, v, self.threads) for a, v in zip(self.kinds, views)):
                host = [views]
        if host is None:
            by_shape: dict = {}
            for s in items:
                f = [read_rgb_uint8(getattr(s, a)) for a in self.kinds]
                if any(a.shape != f[0].shape for a in f):
                    raise ValueError(f"frame sizes differ for sample {s.left_rgb_path}")
                by_shape.setdefault(f[0].shape, []).append(f)
            host = [tuple(torch.from_numpy(np.stack([f[a] for f in run])) for a in range(len(self.kinds)))
                    for run in by_shape.values()]
        parts = []
        for part in host:
            k, Hs, Ws = (int(v) for v in part[0].shape[:3])
            key = (Hs, Ws)
            if key not in self._dev or self._dev[key][0].shape[0] < k:
                self._dev[key] = tuple(torch.empty(max(k, self.bmax), Hs, Ws, 3, dtype=torch.uint8, device=self.device)
                                       for _ in self.kinds)
            up = tuple(d[:k] for d in self._dev[key])
            for d, h in zip(up, part):
                d.copy_(h, non_blocking=h.is_pinned())
            parts.append(up)
        return parts


class _InputLoader:
    """Batches ``{"input": float32 [n, 6, H, W]}`` for ``adapt_epoch``: frames from disk through ``sd_stereo_preprocess``
    at the model's size, the left frame standing in for the label (target and valid are not used)."""

    def __init__(self, frames: _Frames, batches, H: int, W: int, order):
        self.frames, self.batches, self.H, self.W, self.order = frames, batches, H, W, order
        dev, bmax = frames.device, frames.bmax
        self.input = torch.empty(bmax, 6, H, W, device=dev)
        self._target = torch.empty(bmax, 1, H, W, device=dev)
        self._valid = torch.empty(bmax, 1, H, W, device=dev, dtype=torch.bool)

    def __iter__(self):
        dev = self.frames.device
        for i in self.order:
            hw, items = self.batches[i]
            for part in self.frames.load(hw, items):
                n, Hs, Ws = (int(v) for v in part[0].shape[:3])
                with torch.cuda.device(dev):
                    L.call("sd_stereo_preprocess", part[0].data_ptr(), part[1].data_ptr(), part[0].data_ptr(), n, Hs, Ws,
                           self.H, self.W, self.input.data_ptr(), self._target.data_ptr(), self._valid.data_ptr(),
                           L.stream_handle(dev))
                yield {"input": self.input[:n]}


UNCERT_STEPS = 20  # cuts of the sparsification curves of --eval-uncertainty


def _measure_epe(model, frames: _Frames, batches, H: int, W: int, eval_uncertainty: bool = False) -> tuple:
    """EPE and the other figures of ``predict.metrics_from_row`` over every sample, in eval mode (``Predictor.run`` with
    the ground truth and no images: ``sd_disp_export``'s metric rows), and with ``eval_uncertainty`` the figures of
    ``uncert.aggregate_rows`` from the same forward (``sd_uncert_eval``), else None."""
    from .predict import Predictor, aggregate_rows
    from .uncert import UncertaintyEval, aggregate_rows as aggregate_uncert_rows

    pred = Predictor(model, (W, H))  # puts the model into eval mode
    uncert = UncertaintyEval(UNCERT_STEPS, pred.device) if eval_uncertainty else None
    rows, urows = [], []
    for hw, items in batches:
        for part in frames.load(hw, items):
            res = pred.run(part[0], part[1], part[2], images=False, **({"uncert": uncert} if uncert else {}))
            rows.append(res["rows"].cpu().numpy().copy())
            if uncert is not None:
                urows.append(res["urows"].cpu().numpy().copy())
    return (aggregate_rows(np.concatenate(rows)),
            aggregate_uncert_rows(np.concatenate(urows), UNCERT_STEPS) if uncert is not None else None)


def _train_config(ck: dict, opts: dict):
    """A ``cli.TrainConfig`` for the adapted checkpoint: the source checkpoint's args (the trainer's defaults where it
    has none) with what the adaptation changed."""
    from .cli import TrainConfig, build_parser as train_parser

    cfg = vars(train_parser().parse_args([]))
    cfg.update({k: v for k, v in (ck.get("args") or {}).items() if k in cfg})
    cfg.update(height=opts["height"], width=opts["width"], epochs=opts["epochs"], batch_size=opts["batch_size"],
               lr=opts["lr"], weight_decay=opts["weight_decay"], max_samples=opts["max_samples"], seed=opts["seed"],
               precision=opts["precision"], output_dir=opts["output_dir"], resume=None)
    if opts["dataset_root"] is not None:
        cfg["dataset_root"] = opts["dataset_root"]
    return TrainConfig(**cfg)


def adapt(checkpoint, *, model=None, device="cuda", **options) -> dict:
    """The tool as a function: ``options`` are ``adapt_options``' keywords. ``model``: a StereoUNet to adapt instead of
    loading ``checkpoint`` (height and width are then required). Returns the dict that is also written to
    ``adapt_meta.json`` and printed as one JSON line."""
    from .cache import plan_batches
    from .cli import load_checkpoint, save_checkpoint, set_seed
    from .model import StereoUNet
    from .optim import FusedAdamW
    from .predict import dataset_items, pair_by_stem

    opts = adapt_options(**options)
    dev = _resolve_device(device)
    has_gt = opts["dataset_root"] is not None
    if has_gt:
        items = dataset_items(Path(opts["dataset_root"]).expanduser().resolve())
        source = opts["dataset_root"]
    else:
        items = pair_by_stem(opts["left_dir"], opts["right_dir"])
        source = f"{opts['left_dir']} + {opts['right_dir']}"
    if opts["max_samples"] > 0:
        items = items[:opts["max_samples"]]
    if not items:
        raise ValueError(f"No samples discovered under: {source}")

    started_at = time.time()
    set_seed(opts["seed"])
    ck: dict = {}
    if model is None:
        model = StereoUNet(in_channels=6, out_channels=1, base_channels=opts["base_channels"], precision=opts["precision"])
        ck = load_checkpoint(checkpoint, model, None, dev)
        ck_args = ck.get("args") or {}
        if opts["height"] is None:
            opts["height"], opts["width"] = ck_args.get("height"), ck_args.get("width")
    else:
        if getattr(model, "precision", None) == "fp8":
            raise RuntimeError("adapt: precision='fp8' is the inference-only forward; adapt in fp32 or bf16")
        if next(model.parameters()).device.type != "cuda":
            model = model.to(dev)
        opts["precision"], opts["base_channels"] = model.precision, model.base_channels
    H, W = opts["height"], opts["width"]
    if H is None or W is None:
        raise ValueError("--height / --width: the checkpoint carries no args to take them from; pass both.")
    if H <= 0 or W <= 0 or H % 16 or W % 16:
        raise ValueError(f"--height / --width must be positive multiples of 16, got: {H} x {W}")
    out_dir = Path(opts["output_dir"]).expanduser().resolve()
    out_dir.mkdir(parents=True, exist_ok=True)

    dev = next(model.parameters()).device
    batches = plan_batches(items, opts["batch_size"])
    frames = _Frames(dev, opts["batch_size"], has_gt, opts["read_threads"])
    eval_unc = bool(opts.get("eval_uncertainty"))
    before, unc_before = _measure_epe(model, frames, batches, H, W, eval_unc) if has_gt else (None, None)
    optimizer = FusedAdamW(model.parameters(), lr=opts["lr"], weight_decay=opts["weight_decay"])
    use_proxy = opts.get("proxy_weight", 0.0) > 0
    proxy = None
    if use_proxy:
        from .proxy import ProxyLoss

        check_width(W, 0, opts["proxy_num_disparities"])
        proxy = ProxyLoss(opts["batch_size"], w_proxy=opts["proxy_weight"], uncertainty=opts["uncertainty"], device=dev,
                          num_disparities=opts["proxy_num_disparities"], block_size=opts["proxy_block_size"],
                          mode=opts["proxy_mode"], cost=opts.get("proxy_cost", "bt"),
                          census_window=opts.get("proxy_census_window"))
    loss = None
    if not (use_proxy and opts["proxy_only"]):
        loss = SelfSupLoss(opts["batch_size"], w_smooth=opts["w_smooth"], gamma=opts["edge_gamma"],
                           occ_tol=opts["occ_tol"], uncertainty=opts["uncertainty"], device=dev, ssim=opts["ssim_weight"])
    keys = (META_KEYS + (("ssim",) if opts["ssim_weight"] > 0 else ()) if loss is not None else ()) \
        + (PROXY_META_KEYS if use_proxy else ())
    rng = np.random.default_rng(opts["seed"])
    epochs = []
    for _ in range(opts["epochs"]):
        order = [int(i) for i in rng.permutation(len(batches))]
        means = adapt_epoch(model, _InputLoader(frames, batches, H, W, order), dev, optimizer, loss, proxy=proxy)
        epochs.append({k: means[k] for k in keys})
    after, unc_after = _measure_epe(model, frames, batches, H, W, eval_unc) if has_gt else (None, None)
    model.train(False)
    save_checkpoint(out_dir / "adapted.pt", int(ck.get("epoch", 0)), model, optimizer, _train_config(ck, opts),
                    {f"adapt_{k}": v for k, v in epochs[-1].items() if v is not None},
                    global_step=int(ck.get("global_step", 0)))
    described = loss.describe() if loss is not None else {}
    meta = {"format_version": 1, "checkpoint": str(checkpoint) if checkpoint is not None else None, **opts,
            **{f"loss_{k}": v for k, v in described.items() if k in ("w_photo", "eps", "eps_s")},
            "rectified": True, "num_samples": len(items), "num_batches": len(batches), "epochs_run": epochs,
            "photo_first": epochs[0].get("photo"), "photo_last": epochs[-1].get("photo"),
            **({"ssim_first": epochs[0]["ssim"], "ssim_last": epochs[-1]["ssim"]}
               if opts["ssim_weight"] > 0 and loss is not None else {}),
            **({"proxy_mae_first": epochs[0]["proxy_mae"], "proxy_mae_last": epochs[-1]["proxy_mae"]} if use_proxy else {}),
            "epe_before": before["epe"] if before else None, "epe_after": after["epe"] if after else None,
            **({"uncertainty_before": unc_before, "uncertainty_after": unc_after} if eval_unc else {}),
            "output": str(out_dir / "adapted.pt"), "elapsed_seconds": time.time() - started_at,
            "created_at_unix": time.time()}
    (out_dir / "adapt_meta.json").write_text(json.dumps(meta, indent=2), encoding="utf-8")
    print(json.dumps(meta))
    return meta


def main(argv=None) -> dict:
    parser = build_parser()
    a = parser.parse_args(argv)
    try:
        opts = adapt_options(a.left_dir, a.right_dir, a.dataset_root, a.output_dir, a.height, a.width, a.epochs,
                             a.batch_size, a.lr, a.weight_decay, a.precision, a.w_smooth, a.edge_gamma, a.occ_tol,
                             not a.no_uncertainty, a.max_samples, a.seed, a.base_channels, a.read_threads,
                             a.ssim_weight, proxy_weight=a.proxy_weight, proxy_only=a.proxy_only,
                             proxy_num_disparities=a.proxy_num_disparities, proxy_block_size=a.proxy_block_size,
                             proxy_mode=a.proxy_mode, proxy_cost=a.proxy_cost,
                             proxy_census_window=a.proxy_census_window, eval_uncertainty=a.eval_uncertainty)
    except ValueError as e:
        parser.error(str(e))
    _resolve_device(a.device)
    return adapt(a.checkpoint, device=a.device, **opts)


if __name__ == "__main__":
    main()
