"""Device-event times of gradient accumulation:

    python tools/accum_timing.py [--rounds 40] [--inner 25] [--steps 48] [--windows 5] [--out profiles/grad_accumulate.txt]

1. The launch.  mte_grad_accumulate with assign = 0 (12 B per element: read, read, write) and assign = 1 (8 B: read, write) at the flat
   buffer's real size, and in the same run the plain SGD launch, which moves the same 12 B per element in the same 2:1 read:write mix.
   The launches alternate in one process: every round times each of them once, `inner` back-to-back launches between two events, after a
   warm-up round of every launch.  Reported: median, minimum, quartiles and maximum of the per-launch time, bytes over the median, the share
   of the 8.0 TB/s peak, and the accumulate launch's rate against the plain SGD launch's (expected within 10 %: reported, not tuned).
2. The step.  The T8 synthetic training step (PackNet-SAN 1A, bf16, 8 x 384 x 1280, FusedAdam, eager two-stream schedule) per MICRO-BATCH
   with accumulate_grad_batches = 1 and = 4: `steps` micro-batches per window, a host clock around windows that end in a device
   synchronise, the two settings alternating, after a warm-up window of each.  With k = 4 three of four micro-batches end in accumulate()
   and the fourth in step(): the difference per micro-batch is what accumulation costs or saves.
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
    accum = torch.zeros_like(g)
    sgd_hyper = torch.tensor([1e-4, 0.0, 1.0], dtype=torch.float32).cuda()
    st = K._stream()
    launches = [
        ('sgd plain (mte_sgd_step_dev)', 12, lambda: K.lib.mte_sgd_step_dev(p.data_ptr(), g.data_ptr(), None, n, sgd_hyper.data_ptr(), 0.0, 0.0, 0, 1.0, st)),
        ('grad accumulate, assign = 0', 12, lambda: K.lib.mte_grad_accumulate(accum.data_ptr(), g.data_ptr(), n, 0, st)),
        ('grad accumulate, assign = 1', 8, lambda: K.lib.mte_grad_accumulate(accum.data_ptr(), g.data_ptr(), n, 1, st)),
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
    assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(accum).all())
    lines = ['%-34s %5s %8s %8s %8s %8s %8s %7s %6s' % ('launch', 'B/el', 'median', 'min', 'q1', 'q3', 'max', 'TB/s', 'share')]
    rate = {}
    for name, bpe, _ in launches:
        t = sorted(times[name])
        med = statistics.median(t)
        rate[name] = bpe * n / (med * 1e-3) / 1e12
        lines.append('%-34s %5d %8.4f %8.4f %8.4f %8.4f %8.4f %7.2f %5.1f%%' % (name, bpe, med, t[0], t[len(t) // 4], t[(3 * len(t)) // 4], t[-1],
                                                                               rate[name], 100 * rate[name] / PEAK_TBS))
    sgd, acc = rate[launches[0][0]], rate[launches[1][0]]
    verdict = 'within' if acc >= 0.9 * sgd else 'BELOW'
    lines += ['', 'accumulate (assign = 0) runs at %.2f TB/s = %.1f %% of the plain SGD launch\'s %.2f TB/s in this run: %s the 10 %% margin'
              % (acc, 100 * acc / sgd, sgd, verdict),
              'one accumulated micro-batch adds %.4f ms (median of the assign = 0 launch)' % statistics.median(times[launches[1][0]])]
    return lines


def step_times(steps, windows):
    """ms per micro-batch of the T8 synthetic step at k = 1 and k = 4, alternating windows"""
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
    opts = {k: FusedAdam(flat, lr=1e-4, accumulate_grad_batches=k) for k in (1, 4)}

    def window(k):
        opt = opts[k]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            opt.zero_grad()
            if (i + 1) % k:
                with opt.no_sync():
                    model(batch)['loss'].backward()
                opt.accumulate()
            else:
                model(batch)['loss'].backward()
                opt.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    assert steps % 4 == 0, 'whole groups of 4 per window'
    times = {1: [], 4: []}
    for w in range(-1, windows):                             # window -1: warm-up of both settings
        for k in (1, 4):
            ms = window(k)
            if w >= 0:
                times[k].append(ms)
    lines = ['%-28s %8s %8s %8s   %s' % ('setting', 'median', 'min', 'max', 'windows (ms per micro-batch)')]
    for k in (1, 4):
        t = times[k]
        lines.append('%-28s %8.3f %8.3f %8.3f   %s' % ('accumulate_grad_batches = %d' % k, statistics.median(t), min(t), max(t), ' '.join('%.3f' % x for x in t)))
    d = statistics.median(times[4]) - statistics.median(times[1])
    lines += ['', 'k = 4 against k = 1: %+.3f ms per micro-batch (%+.2f %%); k = 1\'s own windows span %.3f ms'
              % (d, 100 * d / statistics.median(times[1]), max(times[1]) - min(times[1]))]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=0, help='elements (default: the flat parameter count of PackNetSAN01 1A)')
    ap.add_argument('--rounds', type=int, default=40)
    ap.add_argument('--inner', type=int, default=25)
    ap.add_argument('--steps', type=int, default=48, help='micro-batches per timed window of the step (a multiple of 4)')
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--no-step', action='store_true', help='the launches only')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'grad_accumulate.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'accum_timing needs an MI355X'
    n = args.n or parameter_count()
    lines = ['gradient accumulation, measured on %s' % torch.cuda.get_device_name(0), '',
             '1. the launch: n = %d fp32 elements (%.1f MB per buffer); %d rounds, launches alternating, %d back-to-back launches per timed window, one '
             'warm-up round' % (n, n * 4 / 1e6, args.rounds, args.inner),
             'device-event ms per launch; TB/s = bytes per element * n / median; share of the %.1f TB/s peak' % PEAK_TBS, '']
    lines += launch_times(n, args.rounds, args.inner)
    if not args.no_step:
        lines += ['', '2. the step: T8 synthetic (PackNet-SAN 1A, bf16, 8 x 384 x 1280, FusedAdam, eager), host clock around windows of %d micro-batches that '
                  'end in a device synchronise; %d windows per setting, alternating, one warm-up window each' % (args.steps, args.windows), '']
        lines += step_times(args.steps, args.windows)
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
