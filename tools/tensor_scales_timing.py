"""Device-event times of the per-tensor multiplier (SEG) steps and the per-tensor statistics launch at the network's real layout
(DESIGN.md 4.23):

    python tools/tensor_scales_timing.py [--rounds 40] [--inner 25] [--out profiles/tensor_scales.txt]

The layout is FlatParameters' of PackNetSAN01 '1A' (218 tensors, each aligned to 64 elements) with the multipliers of
configs/train_packnet_san_kitti_with_edges_finetune.yaml (four classes).  The launches, alternating in one process as
tools/optimizer_timing.py runs them (every round times each once, `inner` back-to-back launches between two events, after a warm-up
round): mte_adamw_step_dev and mte_adamw_step_seg_dev (AdamW, 28 B per parameter), mte_sgd_step_dev and mte_sgd_step_seg_dev (SGD with
momentum, 20 B; the SEG form with Nesterov's look-ahead too, and both without momentum, 12 B: the three momentum instances of the SEG
kernel), mte_grad_norm_clip (4 B) and mte_tensor_stats without and with the weights (4 B and 8 B per parameter read).
Expectations, not bars: the class map adds one byte per 64 elements, so a SEG launch should sit inside its plain launch's own min-max
spread plus 1 %; the statistics launch should be near the norm launch's rate per byte read.  Needs the GPU; there is no fallback."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from mindtheedge_amd import kernels as K  # noqa: E402

PEAK_TBS = 8.0


def layout():
    """(begins, numels, block classes, class scales, total) of the real network under the fine-tuning YAML's rules"""
    import yaml
    from mindtheedge_amd.networks.depth.PackNetSAN01 import PackNetSAN01
    from mindtheedge_amd.trainers.data_parallel import resolve_tensor_scales, tensor_scale_classes
    with torch.device('meta'):
        net = PackNetSAN01(dropout=None, version='1A')
    named = [(n, p) for n, p in net.named_parameters() if p.requires_grad]
    with open(os.path.join(ROOT, 'configs', 'train_packnet_san_kitti_with_edges_finetune.yaml')) as f:
        rules = yaml.safe_load(f)['model']['optimizer']['tensor_scales']
    pairs = resolve_tensor_scales([n for n, _ in named], [tuple(p.shape) for _, p in named], rules)
    classes, class_of = tensor_scale_classes(pairs)
    # FlatParameters' order: reversed, the fusion scalars at the tail (no buffers are made here: the tensors are on the meta device)
    order = list(reversed(range(len(named))))
    order = [i for i in order if named[i][0] not in ('weight', 'bias')] + [i for i in order if named[i][0] in ('weight', 'bias')]
    begins, numels, blocks, total = [], [], [], 0
    for i in order:
        m = named[i][1].numel()
        begins.append(total)
        numels.append(m)
        blocks += [class_of[i]] * ((m + 63) // 64)
        total += (m + 63) // 64 * 64
    return begins, numels, blocks, classes, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=40)
    ap.add_argument('--inner', type=int, default=25)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tensor_scales.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'tensor_scales_timing needs an MI355X'
    begins, numels, blocks, classes, n = layout()
    T = len(begins)
    gen = torch.Generator().manual_seed(0)
    p = torch.randn(n, generator=gen).cuda()
    g = torch.randn(n, generator=gen) * 1e-3
    for b, cnt, nxt in zip(begins, numels, begins[1:] + [n]):
        g[b + cnt:nxt] = 0.0                                 # the padding holds zeros, as in FlatParameters.grad: both sums see the same elements
    g = g.cuda()
    m, v, buf = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    adam_hyper = torch.tensor([1e-4, 1.0 - 0.9 ** 1000, (1.0 - 0.999 ** 1000) ** 0.5], dtype=torch.float64).float().cuda()
    sgd_hyper = torch.tensor([1e-4, 0.9, 1.0], dtype=torch.float32).cuda()
    st = K._stream()
    adam = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, adam_hyper.data_ptr(), 0.9, 0.999, 1e-8)
    sgd = (p.data_ptr(), g.data_ptr(), buf.data_ptr(), n, sgd_hyper.data_ptr(), 0.9)
    sgd0 = sgd[:5] + (0.0,)                                  # momentum 0: `buf` is neither read nor written
    cls = torch.tensor(blocks, dtype=torch.uint8).cuda()
    scales = torch.tensor([x for pair in classes for x in pair], dtype=torch.float32).cuda()
    seg = (cls.data_ptr(), scales.data_ptr(), len(classes), None)
    norm_ctl = torch.zeros(4, dtype=torch.float32).cuda()
    norm_work = torch.zeros((K.lib.mte_grad_norm_work_bytes(n) + 7) // 8, dtype=torch.float64).cuda()
    begin_d, numel_d = torch.tensor(begins, dtype=torch.int64).cuda(), torch.tensor(numels, dtype=torch.int64).cuda()
    stat_work = torch.zeros((K.lib.mte_tensor_stats_work_bytes(n, T) + 7) // 8, dtype=torch.float64).cuda()
    stat_out = torch.zeros(4 * T, dtype=torch.float64).cuda()

    def stats(with_p):
        K.lib.mte_tensor_stats(g.data_ptr(), p.data_ptr() if with_p else None, n, begin_d.data_ptr(), numel_d.data_ptr(), T, stat_work.data_ptr(),
                               stat_out.data_ptr(), st)

    launches = [
        ('adamw (mte_adamw_step_dev)', 28, lambda: K.lib.mte_adamw_step_dev(*adam, 0.01, 1, 1.0, st)),
        ('adamw, SEG form (4 classes)', 28, lambda: K.lib.mte_adamw_step_seg_dev(*adam, 0.01, 1, 1.0, *seg, st)),
        ('sgd momentum (mte_sgd_step_dev)', 20, lambda: K.lib.mte_sgd_step_dev(*sgd, 0.01, 0, 1.0, st)),
        ('sgd momentum, SEG form (4 classes)', 20, lambda: K.lib.mte_sgd_step_seg_dev(*sgd, 0.01, 0, 1.0, *seg, st)),
        ('sgd Nesterov, SEG form (4 classes)', 20, lambda: K.lib.mte_sgd_step_seg_dev(*sgd, 0.01, 1, 1.0, *seg, st)),
        ('sgd plain (mte_sgd_step_dev, momentum 0)', 12, lambda: K.lib.mte_sgd_step_dev(*sgd0, 0.01, 0, 1.0, st)),
        ('sgd plain, SEG form (4 classes)', 12, lambda: K.lib.mte_sgd_step_seg_dev(*sgd0, 0.01, 0, 1.0, *seg, st)),
        ('grad norm + clip coefficient', 4, lambda: K.lib.mte_grad_norm_clip(g.data_ptr(), n, 1.0, 1.0, 1, norm_work.data_ptr(), norm_ctl.data_ptr(), st)),
        ('tensor stats, gradient only', 4, lambda: stats(False)),
        ('tensor stats, gradient and weights', 8, lambda: stats(True)),
    ]
    plain_of = {'adamw, SEG form (4 classes)': 'adamw (mte_adamw_step_dev)', 'sgd momentum, SEG form (4 classes)': 'sgd momentum (mte_sgd_step_dev)',
                'sgd Nesterov, SEG form (4 classes)': 'sgd momentum (mte_sgd_step_dev)', 'sgd plain, SEG form (4 classes)': 'sgd plain (mte_sgd_step_dev, momentum 0)'}
    times = {name: [] for name, _, _ in launches}
    for rnd in range(-1, args.rounds):                       # round -1: warm-up of every launch
        for name, _, fn in launches:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.inner):
                fn()
            e1.record()
            e1.synchronize()
            if rnd >= 0:
                times[name].append(e0.elapsed_time(e1) / args.inner)
    assert bool(torch.isfinite(p).all())
    S_stats, S_norm = float(stat_out.view(-1, 4)[:, 0].sum()), float(norm_work[0])
    lines = ['per-tensor multipliers (SEG steps) and per-tensor statistics, device-event times on %s' % torch.cuda.get_device_name(0),
             'layout: %d tensors, n = %d fp32 elements (%.1f MB per buffer), %d classes, class map %d bytes, %d statistics chunks at most'
             % (T, n, n * 4 / 1e6, len(classes), cls.numel(), n // 32768 + T),
             '%d rounds, launches alternating, %d back-to-back launches per timed window, one warm-up round' % (args.rounds, args.inner),
             'ms per launch; TB/s = bytes per parameter * n / median; share of the %.1f TB/s peak' % PEAK_TBS, '',
             '%-40s %5s %8s %8s %8s %8s %8s %7s %6s' % ('launch', 'B/par', 'median', 'min', 'q1', 'q3', 'max', 'TB/s', 'share')]
    verdicts, rate = [], {}
    for name, bpp, _ in launches:
        t = sorted(times[name])
        med = statistics.median(t)
        q1, q3 = t[len(t) // 4], t[(3 * len(t)) // 4]
        rate[name] = bpp * n / (med * 1e-3) / 1e12
        lines.append('%-40s %5d %8.4f %8.4f %8.4f %8.4f %8.4f %7.2f %5.1f%%' % (name, bpp, med, t[0], q1, q3, t[-1], rate[name], 100 * rate[name] / PEAK_TBS))
        if name in plain_of:
            pt = sorted(times[plain_of[name]])
            pmed = statistics.median(pt)
            bar = pt[-1] + 0.01 * pmed
            verdicts.append('%s: median %.4f ms against its plain launch\'s repeats [%.4f, %.4f] (median %.4f, %+.2f %%); spread + 1 %% = %.4f: %s'
                            % (name, med, pt[0], pt[-1], pmed, 100 * (med / pmed - 1), bar,
                               'ABOVE the plain launch\'s spread plus 1 %' if med > bar else 'inside the plain launch\'s spread plus 1 %'))
        elif name.startswith('tensor stats'):
            nr = rate['grad norm + clip coefficient']
            verdicts.append('%s: %.4f ms = %.2f TB/s = %.0f %% of the norm launch\'s rate per byte read in this run (%.2f TB/s)'
                            % (name, med, rate[name], 100 * rate[name] / nr, nr))
    lines += [''] + verdicts + ['', 'sum over tensors of S_g %.17g against the norm launch\'s S %.17g (relative difference %.3g)'
                                % (S_stats, S_norm, abs(S_stats - S_norm) / S_norm)]
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
