"""CLI of the MI355X engine -- drop-in for the reference's main.py (same flags, main.py:22-39).

    python main.py --data DIR --model pcrlv2 --b 32 --epochs 240 --lr 1e-3 --output saved_dir --n luna --d 3 --gpus 0 --ratio 1.0 --amp
    torchrun --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 main.py ... --gpus 0,1,2,3,4,5,6,7      (one process per GPU)

Differences from the reference: `--gpus` selects the visible devices exactly as before, but multi-GPU runs use one
process per GPU (RCCL) instead of nn.DataParallel -- with a plain `python main.py` and several ids in --gpus the script
re-launches itself under torch.distributed.run.  `--momentum/--weight_decay` are parsed as floats.  `--d 2` runs the 2D
ResNet-18 U-Net path (pcrlv2_amd/train_2d.py; no segmentation_models_pytorch / torchvision needed).  `--data synthetic` trains on
generated batches of the reference's shapes (no dataset on disk needed); a LUNA pre-task directory is read by pcrlv2_amd/data.py
(crops from disk, the reference's torchio augmentations restated on the GPU -- parity with torchio unpinned); with `--d 2` an image
directory is read by pcrlv2_amd/data_chest.py (PNGs decoded by the workers, the reference's torchvision chain restated on the GPU at
Pillow's arithmetic; the list is ./train_val_txt/chest_train.txt when it exists, otherwise every *.png under --data).
`--d 2 --phase finetune --encoder_weights CKPT` (or `--phase scratch`) trains the 14-label chest classifier of the reference's README on the LAST
1 - ratio of the training list (pcrlv2_amd/train_finetune.py); every other combination of --d / --phase exits with a message.
"""
import argparse
import os
import subprocess
import sys
import warnings

# flag, default, type (None = store_true), help -- the reference's flags (main.py:22-39) with their defaults
_FLAGS = (
    ("data", "/data1/luchixiang/LUNA16/processed", str, "dataset directory, or 'synthetic'"),
    ("model", "pcrlv2", str, "model family"),
    ("phase", "pretask", str, "pretask | finetune | scratch"),
    ("b", 16, int, "batch size PER PROCESS"),
    ("epochs", 100, int, "last epoch index (inclusive)"),
    ("lr", 1e-3, float, "initial learning rate"),
    ("output", "./model_genesis_pretrain", str, "checkpoint directory"),
    ("n", "luna", str, "dataset name (goes into the checkpoint file name)"),
    ("d", 3, int, "2 or 3 dimensional model"),
    ("workers", 4, int, "loader workers"),
    ("gpus", "0,1,2,3", str, "visible device ids, comma separated"),
    ("ratio", 0.8, float, "fraction of the data used for pre-training"),
    ("momentum", 0.9, float, "SGD momentum"),
    ("weight_decay", 1e-4, float, "SGD weight decay"),
    ("seed", 42, int, "python/torch seed"),
    ("amp", False, None, "bfloat16 activations and MFMA operands"),
    ("steps_per_epoch", 16, int, "only with --data synthetic"),
    ("resume", "", str, "checkpoint to continue from (model, momentum buffers, epoch)"),
    ("encoder_weights", "", str, "only with --d 2: local ResNet-18 state_dict (torchvision key names) for the encoder; empty = random init "
                                 "(the reference's smp.Unet('resnet18') downloads ImageNet weights, which an offline engine cannot)"),
    ("val_every", 0, int, "held-out validation after every N-th epoch; 0 = never, like the reference.  --d 3: folds 7-9; --d 2: the images of --val_list; "
                          "with --data synthetic a second generated stream"),
    ("save_best", False, None, "with --val_every: write <model>_<n>_<phase>_<ratio>_best.pt whenever the validation total improves strictly "
                               "(--d 3: the model's state_dict; --d 2: the encoder's, the 2D checkpoint layout) plus the metrics under 'val'"),
    ("val_list", "./train_val_txt/chest_valid.txt", str, "only with --d 2 and --val_every > 0: the held-out image list (`name label...` lines, names relative to --data); "
                                                        "a missing list is an error -- the held-out set is never carved out of the training list"),
    ("size2d", 224, int, "only with --d 2 --data synthetic: side of the global views (locals are 96x96)"),
    ("test_list", "./train_val_txt/chest_test.txt", str, "only with --d 2 --phase finetune | scratch: the labelled list evaluated once after the last epoch "
                                                        "(a missing list is an error when it is used)"),
    ("n_class", 14, int, "only with --d 2 --phase finetune | scratch: labels per image (<= 31)"),
    ("dropout", 0.2, float, "only with --d 2 --phase finetune | scratch: dropout in front of the classifier's linear layer"),
)


def build_parser():
    ap = argparse.ArgumentParser(description="PCRLv2 pre-training on MI355X")
    for name, default, kind, text in _FLAGS:
        if kind is None:
            ap.add_argument("--" + name, action="store_true", default=default, help=text)
        else:
            ap.add_argument("--" + name, default=default, type=kind, help=text)
    from . import optim_cli
    optim_cli.add_arguments(ap)       # --optimizer / --betas / --eps / --clip_grad: --d 2 --phase finetune | scratch only
    return ap


class SyntheticLunaLoader:
    """Batches with the contract of datasets/lunaDataset.py:79-81: (input1, input2, gt, gt2, [6 local views]).
    Generated on `device` (the GPU by default: at ~60 ms per b=32 step a CPU generator would be the bottleneck, as the reference's
    CPU augmentation workers are -- SURVEY 8f N3); `train_3d` accepts tensors on either side."""

    def __init__(self, b, steps, seed=0, device=None):
        import torch
        self.device = torch.device(device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu"))
        self.b, self.steps, self.seed, self.g = b, steps, seed, torch.Generator(device=self.device).manual_seed(seed)

    def __len__(self):
        return self.steps

    def reset_rng(self):
        """Back to the first batch of the stream (train_3d.validate: every validation pass sees the same data)."""
        self.g.manual_seed(self.seed)

    def __iter__(self):
        import torch
        kw = dict(generator=self.g, device=self.device)
        for _ in range(self.steps):
            x1 = torch.randn(self.b, 1, 64, 64, 32, **kw)
            x2 = x1 + 0.1 * torch.randn(self.b, 1, 64, 64, 32, **kw)
            gt = torch.rand(self.b, 1, 64, 64, 32, **kw)
            # local views = 16^3 crops of the first global view + noise, as the real loader's are crops of the same volume (lunaDataset.py:60-78) and as
            # SURVEY 8(d) prescribes for loss-curve runs: with i.i.d. noise locals the local cosine term has no signal and its trajectory is chaotic
            # (round 5: bf16 and float32 runs of 2 000 steps ended 0.27 apart in that term alone, profiles/r05_long_run_compare_iid_locals.txt)
            loc = []
            for i in range(6):
                d0, h0, w0 = (i * 9) % 49, (i * 11) % 49, (i * 3) % 17
                loc.append(x1[:, :, d0:d0 + 16, h0:h0 + 16, w0:w0 + 16] + 0.1 * torch.randn(self.b, 1, 16, 16, 16, **kw))
            yield x1, x2, gt, gt, loc


class SyntheticChestLoader(SyntheticLunaLoader):
    """2D batches with the contract train_2d.py:133 consumes: (input1, input2, gt, gt2, [6 local views]) of [b,3,S,S] / [b,3,96,96]."""

    def __init__(self, b, steps, size, seed=0, device=None):
        super().__init__(b, steps, seed, device)
        self.size = size

    def __iter__(self):
        import torch
        kw = dict(generator=self.g, device=self.device)
        for _ in range(self.steps):
            x1 = torch.randn(self.b, 3, self.size, self.size, **kw)
            x2 = x1 + 0.1 * torch.randn(self.b, 3, self.size, self.size, **kw)
            gt = torch.rand(self.b, 3, self.size, self.size, **kw)
            loc = [torch.randn(self.b, 3, 96, 96, **kw) for _ in range(6)]
            yield x1, x2, gt, gt, loc


class SyntheticLabelledChestLoader(SyntheticLunaLoader):
    """Labelled 2D batches for --phase finetune | scratch: (x [b,3,S,S] float32, y [b,K] uint8).  The labels are a FIXED function of the image --
    label k = (mean of channel k % 3 over cell k of a g x g grid, g = ceil(sqrt(K)), is positive) -- and the generator plants a random +-1 offset in
    every cell under the noise, so the function is learnable and both label values occur for every class."""

    def __init__(self, b, steps, size, n_class, seed=0, device=None):
        super().__init__(b, steps, seed, device)
        self.size, self.n_class = size, n_class
        self.sharded = True                        # one stream per rank: nothing to cut

    @staticmethod
    def labels_of(x, n_class):
        import math
        import torch
        g = int(math.ceil(math.sqrt(n_class)))
        S = x.shape[-1]
        c = S // g
        cols = [x[:, k % 3, (k // g) * c:(k // g + 1) * c, (k % g) * c:(k % g + 1) * c].mean(dim=(1, 2)) > 0 for k in range(n_class)]
        return torch.stack(cols, dim=1).to(torch.uint8)

    def __iter__(self):
        import math
        import torch
        kw = dict(generator=self.g, device=self.device)
        g = int(math.ceil(math.sqrt(self.n_class)))
        c = self.size // g
        for _ in range(self.steps):
            x = 0.5 * torch.randn(self.b, 3, self.size, self.size, **kw)
            sign = (torch.rand(self.b, 3, g, g, **kw) < 0.5).float() * 2 - 1
            x[:, :, :g * c, :g * c] += sign.repeat_interleave(c, dim=2).repeat_interleave(c, dim=3)
            yield x, self.labels_of(x, self.n_class)


def supervised(args):
    return args.phase in ("finetune", "scratch")


def get_dataloader(args):
    """`DataGenerator(args).pcrlv2_luna_pretask()` / `.pcrlv2_chest_pretask()` of the reference (data.py:63-99 / 14-61) -- `--data synthetic`:
    generated batches.  --d 2 --phase finetune | scratch: the labelled loaders {'train', 'eval', 'test'}."""
    if args.d == 2 and supervised(args):
        if args.data == 'synthetic':
            rank = int(os.environ.get("RANK", "0"))
            mk = lambda off: SyntheticLabelledChestLoader(args.b, args.steps_per_epoch, args.size2d, args.n_class, args.seed + off + rank)   # noqa: E731
            return {'train': mk(0), 'eval': mk(7919), 'test': mk(15485)}
        if os.path.isdir(args.data):
            from .data_chest import chest_finetune_loaders
            return chest_finetune_loaders(args)
        raise SystemExit("--d 2 --phase {} needs --data synthetic or a directory of chest X-ray images listed, with their labels, in "
                         "./train_val_txt/chest_train.txt".format(args.phase))
    if args.data == 'synthetic' and args.d == 2:
        rank = int(os.environ.get("RANK", "0"))
        ev = None
        if int(getattr(args, "val_every", 0) or 0) > 0:
            ev = SyntheticChestLoader(args.b, args.steps_per_epoch, args.size2d, args.seed + 7919 + rank)      # another stream than any rank's training data
            ev.sharded = True                                                                                # one stream per rank: nothing to cut
        return {'train': SyntheticChestLoader(args.b, args.steps_per_epoch, args.size2d, args.seed + rank), 'eval': ev}
    if args.data == 'synthetic':
        rank = int(os.environ.get("RANK", "0"))
        ev = SyntheticLunaLoader(args.b, args.steps_per_epoch, args.seed + 7919 + rank)      # another stream than any rank's training data
        ev.sharded = True                                                                  # one stream per rank: nothing to cut
        return {'train': SyntheticLunaLoader(args.b, args.steps_per_epoch, args.seed + rank), 'eval': ev}
    if args.d == 2 and os.path.isdir(args.data):
        from .data_chest import chest_pretask_loaders     # images from disk, the torchvision chain on the GPU (data.py:14-61)
        return chest_pretask_loaders(args)
    if args.n == 'luna' and os.path.isdir(os.path.join(args.data, 'subset0')):
        from .data import luna_pretask_loaders     # raw .npy crops from disk, augmentations on the GPU (pcrlv2_amd/data.py)
        return luna_pretask_loaders(args)
    raise SystemExit("--data must be 'synthetic', a LUNA pre-task directory (subset0..subset9 with <series>_global_<k>.npy / _local_<k>.npy; "
                     "make one from LUNA16 with `python luna_preprocess.py --data LUNA16 --save <dir>`) or, with --d 2, a directory of chest X-ray images (listed in ./train_val_txt/chest_train.txt, "
                     "or every *.png under it)")


def check_route(args):
    """Every (model, d, phase) combination either has a training loop or ends here with a message: no parsed flag silently does nothing."""
    if args.model != 'pcrlv2':
        raise SystemExit("--model {}: only 'pcrlv2' is implemented".format(args.model))
    if args.d not in (2, 3):
        raise SystemExit("--d {}: 2 or 3".format(args.d))
    if args.phase not in ('pretask', 'finetune', 'scratch'):
        raise SystemExit("--phase {}: pretask, finetune or scratch".format(args.phase))
    if args.d == 3 and args.phase != 'pretask':
        raise SystemExit("--d 3 --phase {}: 3D fine-tuning is not implemented; supervised training exists for --d 2 (chest X-ray labels) only".format(args.phase))
    if args.d == 2 and args.phase == 'finetune' and not args.encoder_weights:
        raise SystemExit("--phase finetune needs --encoder_weights (a 2D pre-training checkpoint or a ResNet-18 state_dict); to train the classifier from "
                         "random weights use --phase scratch")
    if args.d == 2 and supervised(args) and not 1 <= args.n_class <= 31:
        raise SystemExit("--n_class {}: 1..31".format(args.n_class))
    from . import optim_cli
    optim_cli.check(args)
    if args.phase == 'pretask':
        optim_cli.check_pretask(args)


def launch(args):
    """In front of every training run: the output directory; with several ids in --gpus and no launcher above, this script again under
    torch.distributed.run, one process per GPU (this process then ends with the launcher's exit code); the visible devices; the loader workers'
    share of the CPUs; the parsed flags on the first line of the log."""
    os.makedirs(args.output, exist_ok=True)
    ids = [g for g in args.gpus.split(',') if g != '']
    if len(ids) > 1 and "WORLD_SIZE" not in os.environ:
        env = dict(os.environ, HIP_VISIBLE_DEVICES=args.gpus, HSA_ENABLE_IPC_MODE_LEGACY="0")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={len(ids)}", "--master-addr", "127.0.0.1",
               "--master-port", os.environ.get("MASTER_PORT", "29511"), os.path.abspath(sys.argv[0])] + sys.argv[1:]
        raise SystemExit(subprocess.call(cmd, env=env))
    if "WORLD_SIZE" not in os.environ:
        os.environ["HIP_VISIBLE_DEVICES"] = args.gpus
    os.environ.setdefault("PCRL_LOADER_WORKERS", str(args.workers))     # ddp.bind_rank_to_numa keeps this many CPUs of the rank's share for the loader workers
    print(args)


def main(argv=None):
    warnings.filterwarnings('ignore')       # the command line's choice (the reference's main.py:10), not an importer's
    args = build_parser().parse_args(argv)
    check_route(args)
    launch(args)
    data_loader = get_dataloader(args)
    if args.model == 'pcrlv2' and args.phase == 'pretask' and args.d == 3:
        from .train_3d import train_pcrlv2_3d
        train_pcrlv2_3d(args, data_loader)
    elif args.model == 'pcrlv2' and args.phase == 'pretask' and args.d == 2:
        from .train_2d import train_pcrlv2
        train_pcrlv2(args, data_loader)
    elif args.model == 'pcrlv2' and supervised(args) and args.d == 2:
        from .train_finetune import train_chest_classifier
        train_chest_classifier(args, data_loader)
    else:       # check_route lets nothing else through; a combination added there without a loop must not fall through silently
        raise SystemExit("no training loop for --model {} --d {} --phase {}".format(args.model, args.d, args.phase))


if __name__ == '__main__':
    main()
