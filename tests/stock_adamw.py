"""Stock torch.optim.AdamW on CPU clones as the reference of the InnerAdamW tests. TEST
INFRASTRUCTURE.

One fact about this reference decides how θ can be compared with it: this torch build's CPU
sqrt is not correctly rounded. It is 1 ulp off the IEEE value for about 0.65 % of its
arguments, at every tensor size and layout (tests/test_adamw_cpu.py::
test_restatement_pins_torch_cpu_adamw met it at the long sizes), while the contract of the HIP
kernels -- and numpy's sqrt, which restates it -- is the correctly rounded one. exp_avg,
exp_avg_sq and step never pass through the sqrt; θ does, and a denominator 1 ulp off flips the
rounding of θ + update for a few elements in ten thousand. So the reference is run twice:

  raw    torch.optim.AdamW(foreach=False) exactly as torch ships it. exp_avg, exp_avg_sq and
         step must equal it bit for bit, and θ must at every element whose exp_avg_sq torch's
         own sqrt has rounded correctly in every step so far (the others are counted and
         printed: `suspect`).
  ieee   the same optimizer, the same torch code, with Tensor.sqrt -- the one operation above
         -- replaced by the correctly rounded fp32 square root while it steps. θ, exp_avg,
         exp_avg_sq and step must equal it bit for bit, everywhere.

Figures: in tests/test_inner_adamw_gpu.py::test_dropin_inner_adamw (8,327 elements, four steps,
lr up to 4.5e-4) θ from the GPU differs from `raw` in 0, 1, 3 and 3 elements after steps 1 to
4, all among the 1,456 to 4,351 elements torch's sqrt had rounded 1 ulp off by then, and in
none from `ieee`; in tests/test_inner_adamw_cpu.py::test_four_steps_match_stock_adamw (24,633
elements) in none from either, with 145 to 519 such elements. A plain bit-for-bit comparison
of θ with `raw` alone would pass or fail by the luck of the inputs.
"""
from contextlib import contextmanager

import numpy as np
import torch

_TORCH_SQRT = torch.Tensor.sqrt


def _ieee_sqrt(t, *args, **kw):
    if args or kw or t.dtype != torch.float32 or t.device.type != "cpu":
        return _TORCH_SQRT(t, *args, **kw)
    with np.errstate(all="ignore"):
        return torch.from_numpy(np.sqrt(t.detach().contiguous().numpy())).view(t.shape)


@contextmanager
def ieee_sqrt():
    """While active, Tensor.sqrt of an fp32 CPU tensor is correctly rounded (numpy's)."""
    torch.Tensor.sqrt = _ieee_sqrt
    try:
        yield
    finally:
        torch.Tensor.sqrt = _TORCH_SQRT


def bits(t):
    t = t.detach().cpu().contiguous().view(-1)
    return (t.dtype, t.view(torch.uint8).numpy().tobytes() if t.numel() else b"")


def clones(values):
    return [torch.nn.Parameter(torch.from_numpy(np.array(v, np.float32)).clone())
            for v in values]


class StockPair:
    """The raw and the ieee reference on clones of `values` (arrays shaped like the
    parameters), stepped together on the same gradients."""

    def __init__(self, values, lr_lambda=None, **kw):
        self.raw_p, self.ieee_p = clones(values), clones(values)
        self.raw = torch.optim.AdamW(self.raw_p, foreach=False, **kw)
        self.ieee = torch.optim.AdamW(self.ieee_p, foreach=False, **kw)
        self.scheds = []
        if lr_lambda is not None:
            from torch.optim.lr_scheduler import LambdaLR

            self.scheds = [LambdaLR(self.raw, lr_lambda), LambdaLR(self.ieee, lr_lambda)]
        self.suspect = [torch.zeros(p.shape, dtype=torch.bool) for p in self.raw_p]

    def step(self, grads):
        """grads: CPU tensors or arrays shaped like the parameters (copied)."""
        for params in (self.raw_p, self.ieee_p):
            for p, g in zip(params, grads):
                p.grad = torch.as_tensor(g).detach().cpu().clone().view(p.shape)
        self.raw.step()
        with ieee_sqrt():
            self.ieee.step()
        for s in self.scheds:
            s.step()
        for p, bad in zip(self.raw_p, self.suspect):
            v = self.raw.state[p]["exp_avg_sq"]
            bad |= _TORCH_SQRT(v) != _ieee_sqrt(v)

    def check(self, params, opt, what):
        """params / opt: the optimizer under test and its parameters, after the same steps."""
        n_suspect = n_diff = 0
        for i, (p, r, e, bad) in enumerate(zip(params, self.raw_p, self.ieee_p, self.suspect)):
            s, sr, se = opt.state[p], self.raw.state[r], self.ieee.state[e]
            assert set(s) == set(sr) == {"step", "exp_avg", "exp_avg_sq"}, (what, i)
            for key in ("exp_avg", "exp_avg_sq"):
                assert s[key].shape == p.shape
                assert bits(s[key]) == bits(sr[key]) == bits(se[key]), (what, key, i)
            assert s["step"].dtype == sr["step"].dtype and s["step"].device.type == "cpu"
            assert float(s["step"]) == float(sr["step"]) == float(se["step"]), (what, i)
            got = p.detach().cpu()
            assert bits(got) == bits(e), (what, "theta vs ieee", i, int((got != e.detach()).sum()))
            diff = got != r.detach()
            assert not bool((diff & ~bad).any()), (what, "theta vs raw", i)
            n_suspect += int(bad.sum())
            n_diff += int(diff.sum())
        print(f"{what}: theta equals stock AdamW with the IEEE sqrt everywhere; against stock "
              f"AdamW as shipped it differs in {n_diff} elements, all among the {n_suspect} "
              f"whose exp_avg_sq torch's sqrt rounded 1 ulp off")
