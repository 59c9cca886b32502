"""Device-event times of the weight EMA:

    python tools/ema_timing.py [--rounds 40] [--inner 25] [--steps 24] [--windows 5] [--out profiles/ema.txt]

1. The launches.  mte_ema_update_dev (12 B per element: read e, read p, write e), mte_grad_accumulate with assign = 0 (the same 12 B in the
   same two-reads-one-write mix) and mte_flat_swap (16 B: read both, write both) at the flat buffer's real size.  The launches alternate in
   one process: every round times each of them once, `inner` back-to-back launches between two events, after a warm-up round of every
   launch.  Reported: median, minimum, quartiles and maximum of the per-launch time, bytes over the median, the share of the 8.0 TB/s peak.
   The bar: the EMA launch's median lies within the spread (minimum to maximum) of the accumulate launch's own repeats in this run; where it
   does not, by how much it misses is reported and nothing is tuned.  The swap has no bar.
2. The step.  The T8 synthetic training step (PackNet-SAN 1A, bf16, 8 x 384 x 1280, FusedAdam, eager two-stream schedule) with ema_decay
   off and on: `steps` steps per window, a host clock around windows that end in a device synchronise, the two settings alternating on the
   same weights, after a warm-up window of each.  The difference per step is what the average costs.
Needs the GPU; there is no fallback."""
import argparse
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")            # see mindtheedge_amd/__init__.py
import torch  # noqa: E402
from mindtheedge_amd import kernels as K  # noqa: E402

PEAK_TBS = 8.0


def parameter_count():
    """elements of the flat buffer FlatParameters makes of PackNetSAN01 '1A' (each tensor padded to 64 elements)"""
    from mindtheedge_amd.networks.depth.PackNetSAN01 import PackNetSAN01
    with torch.device('meta'):
        net = PackNetSAN01(dropout=None, version='1A')
    return sum((p.numel() + 63) // 64 * 64 for p in net.parameters() if p.requires_grad)


def launch_times(n, rounds, inner):
    gen = torch.Generator().manual_seed(0)
    p = torch.randn(n, generator=gen).cuda()
    g = (torch.randn(n, generator=gen) * 1e-3).cuda()
    ema, accum = p.clone(), torch.zeros_like(g)
    scal = torch.tensor([0.999, 0.001], dtype=torch.float32).cuda()
    st = K._stream()
    launches = [
        ('grad accumulate, assign = 0', 12, lambda: K.lib.mte_grad_accumulate(accum.data_ptr(), g.data_ptr(), n, 0, st)),
        ('ema update (mte_ema_update_dev)', 12, lambda: K.lib.mte_ema_update_dev(ema.data_ptr(), p.data_ptr(), n, scal.data_ptr(), None, st)),
        ('flat swap (mte_flat_swap)', 16, lambda: K.lib.mte_flat_swap(ema.data_ptr(), accum.data_ptr(), n, st)),
    ]
    assert inner % 2 == 0, 'an even number of swaps per window leaves the buffers where they were'
    times = {name: [] for name, _, _ in launches}
    for rnd in range(-1, rounds):                            # round -1: warm-up of every launch
        for name, _, fn in launches:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            if rnd >= 0:
                times[name].append(e0.elapsed_time(e1) / inner)
    assert bool(torch.isfinite(ema).all()) and bool(torch.isfinite(accum).all())
    lines = ['%-34s %5s %8s %8s %8s %8s %8s %7s %6s' % ('launch', 'B/el', 'median', 'min', 'q1', 'q3', 'max', 'TB/s', 'share')]
    med = {}
    for name, bpe, _ in launches:
        t = sorted(times[name])
        med[name] = statistics.median(t)
        rate = bpe * n / (med[name] * 1e-3) / 1e12
        lines.append('%-34s %5d %8.4f %8.4f %8.4f %8.4f %8.4f %7.2f %5.1f%%' % (name, bpe, med[name], t[0], t[len(t) // 4], t[(3 * len(t)) // 4], t[-1],
                                                                               rate, 100 * rate / PEAK_TBS))
    acc, e = sorted(times[launches[0][0]]), med[launches[1][0]]
    if acc[0] <= e <= acc[-1]:
        verdict = 'INSIDE the spread of the accumulate launch\'s own repeats'
    else:
        miss = e - acc[-1] if e > acc[-1] else e - acc[0]
        verdict = 'OUTSIDE the spread of the accumulate launch\'s own repeats by %+.4f ms (%+.2f %% of its median)' % (miss, 100 * miss / med[launches[0][0]])
    lines += ['', 'ema update: median %.4f ms against the accumulate launch\'s %.4f ms (its repeats span %.4f .. %.4f ms): %s'
              % (e, med[launches[0][0]], acc[0], acc[-1], verdict),
              'one step with ema_decay on adds one such launch; one ema_weights() block adds two swap launches of %.4f ms' % med[launches[2][0]]]
    return lines


def step_times(steps, windows):
    """ms per step of the T8 synthetic step with ema_decay off and on, alternating windows"""
    from mindtheedge_amd.networks.depth.PackNetSAN01 import PackNetSAN01
    from mindtheedge_amd.models.SemiSupEdgeModel import SemiSupEdgeModel
    from mindtheedge_amd.losses.grad_loss import GradLoss
    from mindtheedge_amd.trainers.data_parallel import FlatParameters, FusedAdam
    from mindtheedge_amd.utils.synthetic import synthetic_batch
    dev = torch.device('cuda', torch.cuda.current_device())
    K.set_compute_dtype('bf16')
    batch = synthetic_batch(8, 384, 1280, 1234, dev)
    torch.manual_seed(42)
    random.seed(100)
    net = PackNetSAN01(dropout=0.5, version='1A').to(dev)
    model = SemiSupEdgeModel(supervised_loss_weight=1.0, depth_edges_loss_weight=1.0, supervised_method='sparse-silog',
                             supervised_num_scales=1, edges_depth_edge_loss_all_scales=True, flip_lr_prob=0.5)
    model.add_depth_net(net)
    model.add_edge_loss(GradLoss('cross_entropy', True, [], 10.0, 1.0))
    model.train()
    # one network, one pair of flat buffers, two optimizers over them (each with its own moments): the windows of the two settings alternate
    # on the same weights, and the weight-pack prefetch has one network's packs to rebuild
    flat = FlatParameters(net.parameters())
    opts = {d: FusedAdam(flat, lr=1e-4, ema_decay=d) for d in (0.0, 0.999)}

    def window(d):
        opt = opts[d]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            opt.zero_grad()
            model(batch)['loss'].backward()
            opt.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    times = {0.0: [], 0.999: []}
    for w in range(-1, windows):                             # window -1: warm-up of both settings
        for d in (0.0, 0.999):
            ms = window(d)
            if w >= 0:
                times[d].append(ms)
    lines = ['%-28s %8s %8s %8s   %s' % ('setting', 'median', 'min', 'max', 'windows (ms per step)')]
    for d in (0.0, 0.999):
        t = times[d]
        lines.append('%-28s %8.3f %8.3f %8.3f   %s' % ('ema_decay = %g' % d, statistics.median(t), min(t), max(t), ' '.join('%.3f' % x for x in t)))
    diff = statistics.median(times[0.999]) - statistics.median(times[0.0])
    lines += ['', 'ema_decay on against off: %+.3f ms per step (%+.2f %%); the off setting\'s own windows span %.3f ms'
              % (diff, 100 * diff / statistics.median(times[0.0]), max(times[0.0]) - min(times[0.0]))]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=0, help='elements (default: the flat parameter count of PackNetSAN01 1A)')
    ap.add_argument('--rounds', type=int, default=40)
    ap.add_argument('--inner', type=int, default=24)
    ap.add_argument('--steps', type=int, default=24, help='steps per timed window of the step')
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--no-step', action='store_true', help='the launches only')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ema.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'ema_timing needs an MI355X'
    n = args.n or parameter_count()
    lines = ['weight EMA, measured on %s' % torch.cuda.get_device_name(0), '',
             '1. the launches: n = %d fp32 elements (%.1f MB per buffer); %d rounds, launches alternating, %d back-to-back launches per timed window, one '
             'warm-up round' % (n, n * 4 / 1e6, args.rounds, args.inner),
             'device-event ms per launch; TB/s = bytes per element * n / median; share of the %.1f TB/s peak' % PEAK_TBS, '']
    lines += launch_times(n, args.rounds, args.inner)
    if not args.no_step:
        lines += ['', '2. the step: T8 synthetic (PackNet-SAN 1A, bf16, 8 x 384 x 1280, FusedAdam, eager), host clock around windows of %d steps that '
                  'end in a device synchronise; %d windows per setting, alternating, one warm-up window each' % (args.steps, args.windows), '']
        lines += step_times(args.steps, args.windows)
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
