"""Writes tests/golden/mrstft.npz from the UNMODIFIED reference (MultiResolutionSTFTLoss of its `src/loss.py`), fp32 and
float64, on the CPU.

    python tests/golden/make_golden_mrstft.py [REFERENCE_SRC]     # default: the directory make_golden.py reads

Runs only where the reference checkout exists; the tests read the fixture, never the reference.  Per case
(tests/cases_mrstft.case_ids) and precision (32 / 64):
  <case>_loss<bits>            the loss
  <case>_comp<bits>            (n_res, 2) spectral-convergence and log-magnitude terms
and per term t in full / sc / log (the gradient of the whole loss, of the spectral-convergence terms alone, of the
log-magnitude terms alone -- each divided by the number of resolutions, as in the loss):
  <case>_g<t><bits>            the gradient to x at cases_mrstft.grad_samples (2048 values)
  <case>_g<t>_norm64           l2 norm of the whole float64 gradient
  <case>_g<t>_dist             l2 distance of the whole fp32 gradient from the float64 one
(The sample is smaller than the TCN fixtures': three gradients x ten cases x two precisions have to fit one committed
file.  The GPU tests compare WHOLE gradients against backend="torch", which the CPU tests pin to these values.)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def reference_src():
    if len(sys.argv) > 1:
        return sys.argv[1]
    import re
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "make_golden.py")).read()
    return re.search(r'sys\.path\.insert\(0, "([^"]*/src)"\)', text).group(1)


sys.path.insert(0, reference_src())

import cases_mrstft as cm  # noqa: E402
import loss as ref  # noqa: E402  (reference)


def evaluate(m, x, y, dtype):
    """loss, components and the three gradients with the reference's own methods."""
    x = x.to(dtype).requires_grad_(True)
    y = y.to(dtype)
    loss = m(x, y)
    gfull, = torch.autograd.grad(loss, x)
    sc, lg = [], []
    for n, h, w in zip(m.fft_sizes, m.hop_sizes, m.win_sizes):
        xm, ym = torch.abs(m.stft(x, n, h, w)), torch.abs(m.stft(y, n, h, w))
        sc.append(m.spectral_convergence(xm, ym))
        lg.append(m.log_stft_magnitude(xm, ym))
    gsc, = torch.autograd.grad(sum(sc) / len(sc), x, retain_graph=True)
    glog, = torch.autograd.grad(sum(lg) / len(lg), x)
    comp = torch.stack([torch.stack(sc), torch.stack(lg)], 1).detach()
    return loss.detach(), comp, {"full": gfull, "sc": gsc, "log": glog}


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    m = ref.MultiResolutionSTFTLoss()
    out = {}
    for case in cm.case_ids():
        x, y = cm.inputs(case)
        l32, c32, g32 = evaluate(m, x, y, torch.float32)
        l64, c64, g64 = evaluate(m, x, y, torch.float64)
        out[f"{case}_loss32"], out[f"{case}_loss64"] = l32.numpy(), l64.numpy()
        out[f"{case}_comp32"], out[f"{case}_comp64"] = c32.numpy(), c64.numpy()
        row = [f"loss {abs(l32.item() - l64.item()) / abs(l64.item()):.1e}"]
        for t in cm.TERMS:
            a, b = g32[t].numpy(), g64[t].numpy()
            out[f"{case}_g{t}32"] = cm.grad_samples(a).astype(np.float32)
            out[f"{case}_g{t}64"] = cm.grad_samples(b)
            out[f"{case}_g{t}_norm64"] = np.array(cm.l2(b))
            out[f"{case}_g{t}_dist"] = np.array(cm.l2(a.astype(np.float64) - b))
            row.append(f"g{t} {cm.l2(a.astype(np.float64) - b) / cm.l2(b):.1e}")
        print(f"{case}: reference fp32 vs f64: " + ", ".join(row), flush=True)
    np.savez(cm.GOLDEN, **out)
    print(f"{os.path.getsize(cm.GOLDEN) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
