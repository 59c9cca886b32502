"""Device-event times of the optimizer launches at the network's parameter count (optimizer family):

    python tools/optimizer_timing.py [--rounds 40] [--inner 25] [--out profiles/optimizer_family.txt]

The launches, all in their device-scalar form on the same flat buffers: mte_adam_step_dev (the default step, untouched by the family) and,
from csrc/optim.hip, Adam + L2, AdamW, plain SGD, SGD with momentum, SGD with Nesterov momentum; then the gradient-norm launch of a clipped
or guarded step (mte_grad_norm_clip: reads the gradient once, 4 B per parameter) and the `_ctl_dev` forms of Adam, AdamW and SGD with
momentum, which read the clip coefficient and the skip flag that launch leaves (ctl = {1, 0} here: the plain step's arithmetic), each
reported against its plain counterpart of the same run.  The launches alternate in one process:
every round times each of them once, `inner` back-to-back launches between two events, after a warm-up round of every launch.  Reported per
launch: median, minimum, maximum and quartiles of the per-launch time over the rounds, the bytes the algorithm moves per parameter
(28 / 28 / 28 / 12 / 20 / 20) over the median, and that rate's share of the 8.0 TB/s peak (HBM-bound: the arithmetic is far below the vector rate).
The yardstick is the default Adam launch of the same run: a 28-byte variant counts as slower when its median lies above the default's slowest
repeat.  Needs the GPU; there is no fallback."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from mindtheedge_amd import kernels as K  # noqa: E402

PEAK_TBS = 8.0


def parameter_count():
    """elements of the flat buffer FlatParameters makes of PackNetSAN01 '1A' (each tensor padded to 64 elements)"""
    from mindtheedge_amd.networks.depth.PackNetSAN01 import PackNetSAN01
    with torch.device('meta'):
        net = PackNetSAN01(dropout=None, version='1A')
    return sum((p.numel() + 63) // 64 * 64 for p in net.parameters() if p.requires_grad)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=0, help='elements (default: the flat parameter count of PackNetSAN01 1A)')
    ap.add_argument('--rounds', type=int, default=40)
    ap.add_argument('--inner', type=int, default=25)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'optimizer_family.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'optimizer_timing needs an MI355X'
    n = args.n or parameter_count()
    gen = torch.Generator().manual_seed(0)
    p = torch.randn(n, generator=gen).cuda()
    g = (torch.randn(n, generator=gen) * 1e-3).cuda()
    m, v, buf = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    adam_hyper = torch.tensor([1e-4, 1.0 - 0.9 ** 1000, (1.0 - 0.999 ** 1000) ** 0.5], dtype=torch.float64).float().cuda()
    sgd_hyper = torch.tensor([1e-4, 0.9, 1.0], dtype=torch.float32).cuda()
    st = K._stream()
    adam = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, adam_hyper.data_ptr(), 0.9, 0.999, 1e-8)
    sgd = (p.data_ptr(), g.data_ptr())
    ctl = torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=torch.float32).cuda()
    norm_ctl = torch.zeros(4, dtype=torch.float32).cuda()
    work = torch.zeros((K.lib.mte_grad_norm_work_bytes(n) + 7) // 8, dtype=torch.float64).cuda()
    launches = [
        ('adam (default step, mte_adam_step_dev)', 28, lambda: K.lib.mte_adam_step_dev(*adam, 1.0, st)),
        ('adam + L2 weight decay', 28, lambda: K.lib.mte_adamw_step_dev(*adam, 0.01, 0, 1.0, st)),
        ('adamw', 28, lambda: K.lib.mte_adamw_step_dev(*adam, 0.01, 1, 1.0, st)),
        ('sgd plain', 12, lambda: K.lib.mte_sgd_step_dev(*sgd, None, n, sgd_hyper.data_ptr(), 0.0, 0.0, 0, 1.0, st)),
        ('sgd momentum', 20, lambda: K.lib.mte_sgd_step_dev(*sgd, buf.data_ptr(), n, sgd_hyper.data_ptr(), 0.9, 0.0, 0, 1.0, st)),
        ('sgd nesterov', 20, lambda: K.lib.mte_sgd_step_dev(*sgd, buf.data_ptr(), n, sgd_hyper.data_ptr(), 0.9, 0.0, 1, 1.0, st)),
        ('grad norm + clip coefficient', 4, lambda: K.lib.mte_grad_norm_clip(g.data_ptr(), n, 1.0, 1.0, 1, work.data_ptr(), norm_ctl.data_ptr(), st)),
        ('adam, ctl form (no weight decay)', 28, lambda: K.lib.mte_adamw_step_ctl_dev(*adam, 0.0, 0, 1.0, ctl.data_ptr(), st)),
        ('adamw, ctl form', 28, lambda: K.lib.mte_adamw_step_ctl_dev(*adam, 0.01, 1, 1.0, ctl.data_ptr(), st)),
        ('sgd momentum, ctl form', 20, lambda: K.lib.mte_sgd_step_ctl_dev(*sgd, buf.data_ptr(), n, sgd_hyper.data_ptr(), 0.9, 0.0, 0, 1.0,
                                                                          ctl.data_ptr(), st)),
    ]
    plain_of = {'adam, ctl form (no weight decay)': 'adam (default step, mte_adam_step_dev)', 'adamw, ctl form': 'adamw',
                'sgd momentum, ctl form': 'sgd momentum'}
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
    base = times[launches[0][0]]
    base_med, base_min, base_max = statistics.median(base), min(base), max(base)
    lines = ['optimizer family, device-event times on %s' % torch.cuda.get_device_name(0),
             'n = %d fp32 parameters (%.1f MB per buffer); %d rounds, launches alternating, %d back-to-back launches per timed window, one warm-up round'
             % (n, n * 4 / 1e6, args.rounds, args.inner),
             'ms per launch; TB/s = bytes per parameter * n / median; share of the %.1f TB/s peak' % PEAK_TBS, '',
             '%-40s %5s %8s %8s %8s %8s %8s %7s %6s %9s' % ('launch', 'B/par', 'median', 'min', 'q1', 'q3', 'max', 'TB/s', 'share', 'vs adam')]
    verdicts = []
    for name, bpp, _ in launches:
        t = sorted(times[name])
        med = statistics.median(t)
        q1, q3 = t[len(t) // 4], t[(3 * len(t)) // 4]
        tbs = bpp * n / (med * 1e-3) / 1e12
        lines.append('%-40s %5d %8.4f %8.4f %8.4f %8.4f %8.4f %7.2f %5.1f%% %8.3fx' % (name, bpp, med, t[0], q1, q3, t[-1], tbs, 100 * tbs / PEAK_TBS, med / base_med))
        if name in plain_of:
            pt = sorted(times[plain_of[name]])
            pmed = statistics.median(pt)
            verdicts.append('%s: median %.4f ms against its plain counterpart\'s repeats [%.4f, %.4f] (median %.4f, %+.2f %%): %s'
                            % (name, med, pt[0], pt[-1], pmed, 100 * (med / pmed - 1),
                               'SLOWER than the plain launch beyond its spread' if med > pt[-1] else 'within the spread of the plain launch'))
        elif bpp == 4:
            adam_rate = 28 * n / (base_med * 1e-3) / 1e12
            verdicts.append('%s: %.4f ms = %.2f TB/s = %.0f %% of the rate the default Adam launch reaches in this run (%.2f TB/s); by bytes alone '
                            '4/28 of its %.4f ms would be %.4f ms (reported, no bar); norm %.6g, coefficient %.6g'
                            % (name, med, tbs, 100 * tbs / adam_rate, adam_rate, base_med, base_med * 4 / 28, float(norm_ctl[2]), float(norm_ctl[0])))
        elif bpp == 28 and name != launches[0][0]:
            slower = med > base_max
            verdicts.append('%s: median %.4f ms against the default Adam launch\'s repeats [%.4f, %.4f] (median %.4f): %s'
                            % (name, med, base_min, base_max, base_med, 'SLOWER than the default beyond its spread' if slower else 'within the spread of the default'))
        elif bpp != 28:
            adam_rate = 28 * n / (base_med * 1e-3) / 1e12
            verdicts.append('%s: %.2f TB/s against the default Adam launch\'s %.2f TB/s (%d B against 28 B per parameter; reported, no bar)' % (name, tbs, adam_rate, bpp))
    lines += ['', 'spread of the default Adam launch over its repeats: (max - min) / median = %.2f %%' % (100 * (base_max - base_min) / base_med), ''] + verdicts
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
