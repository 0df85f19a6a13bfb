"""The optimiser options of the fine-tuning command lines (main.py --d 2 --phase finetune | scratch, luna_nodules.py train, seg3d.py train):
--optimizer sgd|adam|adamw, --betas B1,B2, --eps E, --clip_grad F.  Parsing and refusals only: nothing here touches torch or a GPU."""
from __future__ import annotations

KINDS = ("sgd", "adam", "adamw")
DEFAULT_BETAS = "0.9,0.999"


def add_arguments(ap):
    ap.add_argument("--optimizer", default="sgd", help="sgd (momentum, the default) | adam | adamw (decoupled weight decay): fused step kernels over one arena")
    ap.add_argument("--betas", default=DEFAULT_BETAS, help="--optimizer adam | adamw: the two decay rates B1,B2, each in [0, 1)")
    ap.add_argument("--eps", type=float, default=1e-8, help="--optimizer adam | adamw: added to the denominator")
    ap.add_argument("--clip_grad", type=float, default=0.0, help="clip the global L2 norm of the gradients to this value in front of every update "
                    "(after the all-reduce); 0 = off")


def parse_betas(text):
    """'0.9,0.999' -> (0.9, 0.999); anything else exits with a message."""
    parts = [s.strip() for s in str(text).split(",")]
    if len(parts) != 2:
        raise SystemExit(f"--betas {text}: two numbers B1,B2 separated by a comma")
    try:
        betas = tuple(float(s) for s in parts)
    except ValueError:
        raise SystemExit(f"--betas {text}: B1 and B2 are numbers, e.g. {DEFAULT_BETAS}")
    for name, b in zip(("B1", "B2"), betas):
        if not 0.0 <= b < 1.0:
            raise SystemExit(f"--betas {text}: {name} = {b:g} is outside [0, 1)")
    return betas


def check(args):
    """Every refused value exits with its message.  A namespace from before the options existed is an SGD one without clipping."""
    kind = getattr(args, "optimizer", "sgd")
    if kind not in KINDS:
        raise SystemExit(f"--optimizer {kind}: sgd, adam or adamw")
    parse_betas(getattr(args, "betas", DEFAULT_BETAS))
    eps, clip = float(getattr(args, "eps", 1e-8)), float(getattr(args, "clip_grad", 0.0))
    if not eps >= 0:
        raise SystemExit(f"--eps {eps:g}: a non-negative number")
    if not (clip >= 0 and clip != float("inf")):
        raise SystemExit(f"--clip_grad {clip:g}: the largest gradient norm, a positive number; 0 = off")


def check_pretask(args):
    """The pre-task is the reference's SGD with the device-decided divergence guard: no other optimiser, no clipping."""
    kind, clip = getattr(args, "optimizer", "sgd"), float(getattr(args, "clip_grad", 0.0))
    if kind != "sgd":
        raise SystemExit(f"--phase pretask trains with the reference's SGD: --optimizer {kind} is for --phase finetune | scratch")
    if clip != 0:
        raise SystemExit("--phase pretask does not clip gradients (its guard against a diverged step is decided on the device): "
                         "--clip_grad is for --phase finetune | scratch")


def options(args):
    """-> the keywords loop.run_epochs adds to task.make_optimizer's: none at all for plain SGD, so that call is what it always was."""
    kind, clip = getattr(args, "optimizer", "sgd"), float(getattr(args, "clip_grad", 0.0))
    kw = {}
    if kind != "sgd":
        kw.update(kind=kind, betas=parse_betas(getattr(args, "betas", DEFAULT_BETAS)), eps=float(getattr(args, "eps", 1e-8)))
    if clip > 0:
        kw["max_grad_norm"] = clip
    return kw
