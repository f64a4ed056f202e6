"""TensorBoard + console logging (reference federated.py:27-31,
utils.py:287-303).  Scalar names and the run-name format are kept
reference-identical so existing dashboards read both; the build adds
Perf/* scalars (rounds/sec, phase timings)."""

from time import ctime


def run_name(args):
    """Reference federated.py:27-30 run-name string; the trimmed mean, krum,
    geomed, bulyan and foolsgold (build additions) append their own flags,
    every other rule keeps the reference name byte for byte.  Server-side clipping and the
    attack boost (build additions) append theirs only when switched on."""
    name = (f"time:{ctime()}-clip_val:{args.clip}-noise_std:{args.noise}"
            f"-aggr:{args.aggr}-s_lr:{args.server_lr}-num_cor:{args.num_corrupt}"
            f"thrs_robustLR:{args.robustLR_threshold}"
            f"-num_corrupt:{args.num_corrupt}-pttrn:{args.pattern_type}")
    if args.aggr == 'trmean':
        name += f"-trim:{args.trim_frac}"
    if args.aggr == 'krum':
        name += f"-krum_f:{args.krum_f}-krum_m:{args.krum_m}"
    if args.aggr == 'geomed':
        name += f"-gm_iters:{args.geomed_iters}-gm_nu:{args.geomed_nu}"
    if args.aggr == 'bulyan':
        name += f"-bulyan_f:{args.bulyan_f}"
    if args.aggr == 'foolsgold':
        name += f"-fg_kappa:{args.foolsgold_kappa}"
    if getattr(args, 'server_clip', 0) > 0:
        name += f"-sclip:{args.server_clip}-{args.server_clip_mode}"
    if getattr(args, 'attack_boost', 1.0) != 1.0:
        name += f"-boost:{args.attack_boost}"
    return name


def build_writer(args):
    if getattr(args, 'no_tb', False):
        return None
    try:
        from torch.utils.tensorboard import SummaryWriter
    except ImportError:
        return None
    return SummaryWriter(f"{args.log_dir}/{run_name(args)}")


def foolsgold_history_bytes(args):
    """8 * num_agents * n_params: what --aggr foolsgold keeps on the device
    across rounds."""
    from ..models import get_model
    model = get_model(args.data, getattr(args, 'model', None))
    return 8 * args.num_agents * sum(p.numel() for p in model.parameters())


def print_exp_details(args):
    """Reference utils.py:287-303."""
    print('======================================')
    print(f'    Dataset: {args.data}')
    print(f'    Global Rounds: {args.rounds}')
    print(f'    Aggregation Function: {args.aggr}')
    if args.aggr == 'trmean':
        print(f'    Trim Fraction: {args.trim_frac}')
    if args.aggr == 'krum':
        print(f'    Krum f / m: {args.krum_f} / {args.krum_m}')
    if args.aggr == 'geomed':
        print(f'    Geomed iters / nu: {args.geomed_iters} / '
              f'{args.geomed_nu}')
    if args.aggr == 'bulyan':
        print(f'    Bulyan f: {args.bulyan_f}')
    if args.aggr == 'foolsgold':
        print(f'    FoolsGold kappa: {args.foolsgold_kappa} (history '
              f'{foolsgold_history_bytes(args) / 1e6:.0f} MB)')
    if getattr(args, 'server_clip', 0) > 0:
        print(f'    Server Clip: {args.server_clip} '
              f'({args.server_clip_mode})')
    if getattr(args, 'attack_boost', 1.0) != 1.0:
        print(f'    Attack Boost: {args.attack_boost}')
    print(f'    Number of agents: {args.num_agents}')
    print(f'    Fraction of agents: {args.agent_frac}')
    print(f'    Batch size: {args.bs}')
    print(f'    Client_LR: {args.client_lr}')
    print(f'    Server_LR: {args.server_lr}')
    print(f'    Client_Momentum: {args.client_moment}')
    print(f'    RobustLR_threshold: {args.robustLR_threshold}')
    print(f'    Noise Ratio: {args.noise}')
    print(f'    Number of corrupt agents: {args.num_corrupt}')
    print(f'    Poison Frac: {args.poison_frac}')
    print(f'    Clip: {args.clip}')
    print('======================================')
