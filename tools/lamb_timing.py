"""Device-event times of the two LAMB launches at the network's real layout, and the training step with LAMB against AdamW
(DESIGN.md 4.24):

    python tools/lamb_timing.py [--rounds 40] [--inner 25] [--steps 24] [--windows 5] [--no-step] [--out profiles/lamb.txt]

1. The launches.  mte_lamb_moments (24 B per parameter: read p, g, m, v; write m, v) and mte_lamb_apply (16 B: read p, m, v; write p) over
   FlatParameters' layout of PackNetSAN01 '1A' (218 tensors, each aligned to 64 elements) with the default exclusion (the tensors of at
   most one dimension keep AdamW's arithmetic), alternating in one process with the plain AdamW launch (mte_adamw_step_dev, 28 B) and the
   statistics launch whose chunk walk the pair shares (mte_tensor_stats with the weights, 8 B read), as tools/tensor_scales_timing.py
   runs its launches: every round times each once, `inner` back-to-back launches between two events, after a warm-up round.
   The yardstick is bytes: the pair moves 40 B per parameter against AdamW's 28, so the expectation is 40 / 28 of the AdamW time of the
   same run; the moments launch carries the chunk table and the fp64 accumulators that cost the statistics launch about 10 % against
   the norm launch (profiles/tensor_scales.txt), and that shortfall is the margin it gets.  Expectations, not bars.
2. The step.  The T8 synthetic training step (PackNet-SAN 1A, bf16, 8 x 384 x 1280, eager) with FusedAdam (AdamW) and with FusedLAMB over
   the same flat buffers: `steps` steps per window, a host clock around windows that end in a device synchronise, the two alternating,
   after a warm-up window of each (tools/ema_timing.py's scheme).
Needs the GPU; there is no fallback."""
import argparse
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from mindtheedge_amd import kernels as K  # noqa: E402

PEAK_TBS = 8.0


def layout():
    """(begins, numels, {lr_mult, wd_mult, adapt} rows, total) of the real network under the default lamb_exclude"""
    from mindtheedge_amd.networks.depth.PackNetSAN01 import PackNetSAN01
    from mindtheedge_amd.trainers.data_parallel import resolve_lamb_exclude
    with torch.device('meta'):
        net = PackNetSAN01(dropout=None, version='1A')
    named = [(n, p) for n, p in net.named_parameters() if p.requires_grad]
    adapt = resolve_lamb_exclude([n for n, _ in named], [tuple(p.shape) for _, p in named], [{'max_ndim': 1}])
    # FlatParameters' order: reversed, the fusion scalars at the tail (no buffers are made here: the tensors are on the meta device)
    order = list(reversed(range(len(named))))
    order = [i for i in order if named[i][0] not in ('weight', 'bias')] + [i for i in order if named[i][0] in ('weight', 'bias')]
    begins, numels, rows, total = [], [], [], 0
    for i in order:
        m = named[i][1].numel()
        begins.append(total)
        numels.append(m)
        rows += [1.0, 1.0, 1.0 if adapt[i] else 0.0]
        total += (m + 63) // 64 * 64
    return begins, numels, rows, total


def launch_times(rounds, inner):
    begins, numels, rows, n = layout()
    T = len(begins)
    gen = torch.Generator().manual_seed(0)
    p = torch.randn(n, generator=gen).cuda()
    g = (torch.randn(n, generator=gen) * 1e-3).cuda()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    hyper = torch.tensor([1e-4, 1.0 - 0.9 ** 1000, (1.0 - 0.999 ** 1000) ** 0.5], dtype=torch.float64).float().cuda()
    st = K._stream()
    begin_d, numel_d = torch.tensor(begins, dtype=torch.int64).cuda(), torch.tensor(numels, dtype=torch.int64).cuda()
    table = torch.tensor(rows, dtype=torch.float32).cuda()
    work = torch.zeros((K.lib.mte_lamb_work_bytes(n, T) + 7) // 8, dtype=torch.float64).cuda()
    trust, sums = torch.zeros(T, dtype=torch.float32).cuda(), torch.zeros(2 * T, dtype=torch.float64).cuda()
    stat_work = torch.zeros((K.lib.mte_tensor_stats_work_bytes(n, T) + 7) // 8, dtype=torch.float64).cuda()
    stat_out = torch.zeros(4 * T, dtype=torch.float64).cuda()
    tabs = (begin_d.data_ptr(), numel_d.data_ptr(), table.data_ptr(), T)

    def moments():
        K.lib.mte_lamb_moments(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, hyper.data_ptr(), 0.9, 0.999, 1e-8, 0.01, 1.0, 0.0, *tabs,
                               work.data_ptr(), trust.data_ptr(), sums.data_ptr(), None, st)

    def apply():
        K.lib.mte_lamb_apply(p.data_ptr(), m.data_ptr(), v.data_ptr(), n, hyper.data_ptr(), 1e-8, 0.01, *tabs, trust.data_ptr(), None, st)

    launches = [
        ('adamw (mte_adamw_step_dev)', 28, lambda: K.lib.mte_adamw_step_dev(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, hyper.data_ptr(),
                                                                          0.9, 0.999, 1e-8, 0.01, 1, 1.0, st)),
        ('lamb moments (mte_lamb_moments)', 24, moments),
        ('lamb apply (mte_lamb_apply)', 16, apply),
        ('tensor stats, gradient and weights', 8, lambda: K.lib.mte_tensor_stats(g.data_ptr(), p.data_ptr(), n, begin_d.data_ptr(), numel_d.data_ptr(), T,
                                                                                   stat_work.data_ptr(), stat_out.data_ptr(), st)),
    ]
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
    assert bool(torch.isfinite(p).all()) and bool((trust > 0).all())
    lines = ['layout: %d tensors (%d adapted), n = %d fp32 elements (%.1f MB per buffer), %d chunks at most'
             % (T, int(sum(rows[2::3])), n, n * 4 / 1e6, n // 32768 + T),
             '%d rounds, launches alternating, %d back-to-back launches per timed window, one warm-up round' % (rounds, inner),
             'ms per launch; TB/s = bytes per parameter * n / median; share of the %.1f TB/s peak' % PEAK_TBS, '',
             '%-40s %5s %8s %8s %8s %8s %8s %7s %6s' % ('launch', 'B/par', 'median', 'min', 'q1', 'q3', 'max', 'TB/s', 'share')]
    med, rate = {}, {}
    for name, bpp, _ in launches:
        t = sorted(times[name])
        med[name] = statistics.median(t)
        rate[name] = bpp * n / (med[name] * 1e-3) / 1e12
        lines.append('%-40s %5d %8.4f %8.4f %8.4f %8.4f %8.4f %7.2f %5.1f%%' % (name, bpp, med[name], t[0], t[len(t) // 4], t[(3 * len(t)) // 4], t[-1],
                                                                                   rate[name], 100 * rate[name] / PEAK_TBS))
    a, mo, ap_ = (med[launches[i][0]] for i in (0, 1, 2))
    at = sorted(times[launches[0][0]])
    lines += ['', 'the pair: %.4f + %.4f = %.4f ms, 40 B per parameter = %.2f TB/s' % (mo, ap_, mo + ap_, 40 * n / ((mo + ap_) * 1e-3) / 1e12),
              'the AdamW launch of this run: median %.4f ms, repeats [%.4f, %.4f] (spread %.4f ms); 40 / 28 of it = %.4f ms'
              % (a, at[0], at[-1], at[-1] - at[0], a * 40 / 28),
              'the pair against 40 / 28 of AdamW: %+.2f %%;  moments against 24 / 28: %+.2f %%;  apply against 16 / 28: %+.2f %%'
              % (100 * ((mo + ap_) / (a * 40 / 28) - 1), 100 * (mo / (a * 24 / 28) - 1), 100 * (ap_ / (a * 16 / 28) - 1))]
    return lines


def step_times(steps, windows):
    """ms per step of the T8 synthetic step with AdamW and with LAMB, alternating windows over the same flat buffers"""
    from mindtheedge_amd.networks.depth.PackNetSAN01 import PackNetSAN01
    from mindtheedge_amd.models.SemiSupEdgeModel import SemiSupEdgeModel
    from mindtheedge_amd.losses.grad_loss import GradLoss
    from mindtheedge_amd.trainers.data_parallel import FlatParameters, FusedAdam, FusedLAMB
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
    flat = FlatParameters(net.parameters())
    opts = {'AdamW': FusedAdam(flat, lr=1e-4, weight_decay=0.01, decoupled_weight_decay=True),
            'LAMB': FusedLAMB(flat, lr=1e-4, weight_decay=0.01, warmup_steps=500, adapt=[p.dim() > 1 for p in flat.natural_params])}

    def window(name):
        opt = opts[name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            opt.zero_grad()
            model(batch)['loss'].backward()
            opt.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    times = {name: [] for name in opts}
    for w in range(-1, windows):                             # window -1: warm-up of both
        for name in opts:
            ms = window(name)
            if w >= 0:
                times[name].append(ms)
    lines = ['%-28s %8s %8s %8s   %s' % ('optimizer', 'median', 'min', 'max', 'windows (ms per step)')]
    for name, t in times.items():
        lines.append('%-28s %8.3f %8.3f %8.3f   %s' % (name, statistics.median(t), min(t), max(t), ' '.join('%.3f' % x for x in t)))
    diff = statistics.median(times['LAMB']) - statistics.median(times['AdamW'])
    lines += ['', 'LAMB against AdamW: %+.3f ms per step (%+.2f %%); AdamW\'s own windows span %.3f ms'
              % (diff, 100 * diff / statistics.median(times['AdamW']), max(times['AdamW']) - min(times['AdamW']))]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=40)
    ap.add_argument('--inner', type=int, default=25)
    ap.add_argument('--steps', type=int, default=24)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--no-step', action='store_true', help='the launches only')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lamb.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'lamb_timing needs an MI355X'
    lines = ['LAMB: the two fused flat launches and the training step, on %s' % torch.cuda.get_device_name(0), '',
             '1. the launches, device-event times', '']
    lines += launch_times(args.rounds, args.inner)
    if not args.no_step:
        torch.cuda.empty_cache()
        lines += ['', '2. the step: T8 synthetic (PackNet-SAN 1A, bf16, 8 x 384 x 1280, eager), host clock around windows of %d steps that end in a '
                  'device synchronise; %d windows per optimizer, alternating, one warm-up window each' % (args.steps, args.windows), '']
        lines += step_times(args.steps, args.windows)
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
