"""CLI — reproduces the reference's full 21-flag surface
(reference: src/options.py:4-74) plus infrastructure flags that the
MI355X build adds (--seed, --ckpt_dir, --resume, --synthetic, --dtype,
--agents_per_stream, --no_tb), its aggregation rules and their flags, the
server-side norm clip (--server_clip, --server_clip_mode) and the boosted
attack (--attack_boost).

Notes kept behavior-compatible with the reference:
  * default base_class is 5 (options.py:40 — the README's claim of 1 is
    wrong; code wins).
  * the driver forces server_lr = 1 unless aggr == 'sign'
    (reference federated.py:23) — done in finalize_args().
"""

import argparse

SERVER_CLIP_MODES = ('fixed', 'median')


def args_parser(argv=None):
    parser = argparse.ArgumentParser(description="rlr_amd federated trainer")

    # ---- reference flag surface (options.py:7-71) ----
    parser.add_argument('--data', type=str, default='fmnist',
                        help="dataset to train on: fmnist | cifar10 | fedemnist")
    parser.add_argument('--num_agents', type=int, default=10,
                        help="number of agents K")
    parser.add_argument('--agent_frac', type=float, default=1,
                        help="fraction of agents sampled per round C")
    parser.add_argument('--num_corrupt', type=int, default=0,
                        help="number of corrupt agents")
    parser.add_argument('--rounds', type=int, default=200,
                        help="number of communication rounds R")
    parser.add_argument('--aggr', type=str, default='avg',
                        choices=['avg', 'comed', 'sign', 'trmean', 'krum',
                                 'geomed', 'bulyan', 'foolsgold'],
                        help="aggregation rule (trmean, krum, geomed, bulyan "
                             "and foolsgold are build additions)")
    parser.add_argument('--local_ep', type=int, default=2,
                        help="number of local epochs E")
    parser.add_argument('--bs', type=int, default=256,
                        help="local batch size B")
    parser.add_argument('--client_lr', type=float, default=0.1,
                        help="client learning rate")
    parser.add_argument('--client_moment', type=float, default=0.9,
                        help="client momentum")
    parser.add_argument('--server_lr', type=float, default=1,
                        help="server learning rate (signSGD)")
    parser.add_argument('--base_class', type=int, default=5,
                        help="base class for the backdoor attack")
    parser.add_argument('--target_class', type=int, default=7,
                        help="target class for the backdoor attack")
    parser.add_argument('--poison_frac', type=float, default=0.0,
                        help="fraction of a corrupt agent's base-class data to trojan")
    parser.add_argument('--pattern_type', type=str, default='plus',
                        help="trojan pattern: plus | square | copyright | apple")
    parser.add_argument('--robustLR_threshold', type=int, default=0,
                        help="RLR vote threshold theta (0 disables the defense)")
    parser.add_argument('--clip', type=float, default=0,
                        help="L2 ball radius for the per-batch PGD projection (0 disables)")
    parser.add_argument('--noise', type=float, default=0,
                        help="gaussian noise std multiplier (std = noise*clip)")
    parser.add_argument('--top_frac', type=int, default=100,
                        help="number of top-Fisher coords for sign-agreement diagnostics")
    parser.add_argument('--snap', type=int, default=1,
                        help="evaluate every snap rounds")
    parser.add_argument('--device', type=str, default=None,
                        help="device; default cuda:LOCAL_RANK if available else cpu")
    parser.add_argument('--num_workers', type=int, default=0,
                        help="dataloader workers (kept for CLI parity; the GPU path "
                             "keeps datasets resident in HBM and does not use workers)")

    # ---- MI355X build additions ----
    parser.add_argument('--trim_frac', type=float, default=0.1,
                        help="fraction of sampled agents trimmed from each "
                             "end per coordinate (--aggr trmean)")
    parser.add_argument('--krum_f', type=int, default=1,
                        help="number of sampled agents assumed Byzantine "
                             "(--aggr krum)")
    parser.add_argument('--krum_m', type=int, default=0,
                        help="number of agents Krum keeps: 1 = classic Krum, "
                             "0 = K - krum_f (Multi-Krum)")
    parser.add_argument('--bulyan_f', type=int, default=1,
                        help="number of sampled agents assumed Byzantine; "
                             "needs K >= 4 f + 3 (--aggr bulyan)")
    parser.add_argument('--geomed_iters', type=int, default=8,
                        help="smoothed Weiszfeld iterations; 0 = the "
                             "unweighted mean (--aggr geomed)")
    parser.add_argument('--geomed_nu', type=float, default=1e-6,
                        help="smoothing: a weight is 1 / max(nu, distance) "
                             "(--aggr geomed)")
    parser.add_argument('--foolsgold_kappa', type=float, default=1.0,
                        help="confidence of the logit that turns similarity "
                             "into a weight, > 0 (--aggr foolsgold)")
    parser.add_argument('--server_clip', type=float, default=0,
                        help="server-side bound on each update's L2 norm "
                             "before aggregation (0 disables)")
    parser.add_argument('--server_clip_mode', type=str, default='fixed',
                        choices=list(SERVER_CLIP_MODES),
                        help="fixed: --server_clip is the bound; median: it "
                             "multiplies the median norm of the round's "
                             "sampled updates")
    parser.add_argument('--attack_boost', type=float, default=1.0,
                        help="corrupt agents multiply their update by this "
                             "before sending it (model replacement)")
    parser.add_argument('--seed', type=int, default=42,
                        help="master seed; all RNG streams derive from it "
                             "world-size-invariantly")
    parser.add_argument('--ckpt_dir', type=str, default='',
                        help="directory for checkpoints (empty = no checkpointing)")
    parser.add_argument('--resume', type=str, default='',
                        help="path to a checkpoint to resume from")
    parser.add_argument('--synthetic', action='store_true', default=False,
                        help="use deterministic synthetic data shaped like the real "
                             "dataset (no download needed; bench default)")
    parser.add_argument('--dtype', type=str, default='fp32',
                        choices=['fp32', 'bf16'],
                        help="client compute dtype (updates stay fp64 as in the "
                             "reference, agent.py:63)")
    parser.add_argument('--agents_per_stream', type=int, default=0,
                        help="train up to this many agents concurrently on separate "
                             "HIP streams per rank (0 = auto)")
    parser.add_argument('--model', type=str, default=None,
                        choices=[None, 'resnet18'],
                        help="override the dataset->model mapping "
                             "(build extension: ResNet18 w/ BatchNorm)")
    parser.add_argument('--no_tb', action='store_true', default=False,
                        help="disable the TensorBoard writer")
    parser.add_argument('--no_hip_graphs', dest='hip_graphs',
                        action='store_false', default=True,
                        help="disable hipGraph capture of the training step "
                             "(debug; results are bitwise identical either "
                             "way)")
    parser.add_argument('--log_dir', type=str, default='logs',
                        help="TensorBoard log root")

    args = parser.parse_args(argv)
    try:
        return finalize_args(args)
    except ValueError as e:
        parser.error(str(e))


def check_geomed(iters, nu):
    """The K-independent limits of --aggr geomed, for the parser and for a
    server that is handed its args directly."""
    if iters < 0:
        raise ValueError(f"--geomed_iters must be >= 0, got {iters}")
    if not nu > 0:
        raise ValueError(f"--geomed_nu must be > 0, got {nu}")


def check_foolsgold(kappa):
    """Likewise for --aggr foolsgold."""
    if not 0 < kappa < float('inf'):
        raise ValueError(f"--foolsgold_kappa must be > 0, got {kappa}")


def check_server_clip(value, mode):
    """Likewise for the server-side norm clip."""
    if not value >= 0:
        raise ValueError(f"--server_clip must be >= 0, got {value}")
    if mode not in SERVER_CLIP_MODES:
        raise ValueError(
            f"--server_clip_mode must be one of {SERVER_CLIP_MODES}, got "
            f"{mode}")


def finalize_args(args):
    """Derived rules. server_lr forced to 1 unless aggr=='sign'
    (reference federated.py:23); 0 <= trim_frac < 0.5 so that at least one
    value per coordinate survives the trim for every K; krum_f, krum_m >= 0
    (their upper limits depend on the sampled K and are checked by the
    server); bulyan_f >= 0 (K >= 4 bulyan_f + 3 likewise by the server);
    geomed_iters >= 0 and geomed_nu > 0; foolsgold_kappa > 0; server_clip >= 0 with a known mode;
    attack_boost > 0."""
    args.server_lr = args.server_lr if args.aggr == 'sign' else 1.0
    if not 0 <= args.trim_frac < 0.5:
        raise ValueError(
            f"--trim_frac must be in [0, 0.5), got {args.trim_frac}")
    if args.krum_f < 0 or args.krum_m < 0:
        raise ValueError(
            f"--krum_f and --krum_m must be >= 0, got {args.krum_f} and "
            f"{args.krum_m}")
    if args.bulyan_f < 0:
        raise ValueError(f"--bulyan_f must be >= 0, got {args.bulyan_f}")
    check_geomed(args.geomed_iters, args.geomed_nu)
    check_foolsgold(args.foolsgold_kappa)
    check_server_clip(args.server_clip, args.server_clip_mode)
    if not 0 < args.attack_boost < float('inf'):
        raise ValueError(
            f"--attack_boost must be > 0, got {args.attack_boost}")
    if args.device is None:
        import torch
        if torch.cuda.is_available():
            import os
            lr = int(os.environ.get('LOCAL_RANK', 0))
            args.device = f'cuda:{lr}'
        else:
            args.device = 'cpu'
    return args


def default_args(**overrides):
    """Programmatic args (tests, bench): the parser's defaults + overrides."""
    args = args_parser([])
    for k, v in overrides.items():
        if not hasattr(args, k):
            raise AttributeError(f"unknown option {k}")
        setattr(args, k, v)
    return finalize_args(args)
