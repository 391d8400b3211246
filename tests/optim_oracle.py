"""An independent reference for the flat optimizers, and the fixture the oracle tests share.

The oracle is per tensor and float64.  SGD and AdamW are ``torch.optim.SGD`` /
``torch.optim.AdamW`` on float64 clones with two param groups (decay / no decay) and
``torch.nn.utils.clip_grad_norm_``; LAMB is written out per tensor from the paper (You et
al. 2019) as ``optim/flat.py``'s docstring states it.  Nothing here comes from
``optim/flat.py`` or ``ops/_native_optim.py``: a rule spelled wrong in both of the project's
own paths (kernel and torch path) still disagrees with this module.

``dtype=torch.float32`` runs the identical oracle in fp32.  Its distance from the float64 run
is the yardstick of the tests: what a correct fp32 implementation of the same rules costs on
the same inputs.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import torch

MARGIN = 4.0   # allowed multiple of the fp32 oracle's own error (see ``bound``)


# ---------------------------------------------------------------------------- the oracle
def _split(entries, flat: torch.Tensor, dtype) -> List[torch.Tensor]:
    return [flat[e.offset:e.offset + e.numel].detach().cpu().to(dtype).reshape(e.shape).clone() for e in entries]


def run_oracle(kind: str, entries, init: torch.Tensor, grads: Sequence[torch.Tensor], hp: Dict[str, object],
               lrs: Sequence[float], grad_scale: float, dtype=torch.float64) -> List[Dict[str, object]]:
    """``entries``: the arena's entries (``name``, ``offset``, ``numel``, ``shape``, ``decay``);
    ``init``: the flat initial parameters; ``grads``: per-step flat gradients exactly as handed
    to ``opt.step`` (already rounded to the gradient dtype); ``lrs``: the learning rate of each
    step.  Returns, per step, ``{"params": [...], "state": {name: [...]}, "norm": float}`` with
    per-tensor tensors of ``dtype`` and the pre-clip global gradient norm."""
    params = [torch.nn.Parameter(t) for t in _split(entries, init, dtype)]
    wd = float(hp.get("weight_decay", 0.0))
    max_norm = float(hp.get("max_grad_norm", 0.0) or 0.0)
    groups = [{"params": [p for p, e in zip(params, entries) if e.decay], "weight_decay": wd},
              {"params": [p for p, e in zip(params, entries) if not e.decay], "weight_decay": 0.0}]
    groups = [g for g in groups if g["params"]]
    if kind == "sgd":
        opt = torch.optim.SGD(groups, lr=lrs[0], momentum=hp["momentum"], nesterov=bool(hp.get("nesterov", False)),
                              foreach=False)
    elif kind == "adamw":
        opt = torch.optim.AdamW(groups, lr=lrs[0], betas=tuple(hp["betas"]), eps=hp["eps"], foreach=False)
    elif kind == "lamb":
        opt = None
        m = [torch.zeros_like(p) for p in params]
        v = [torch.zeros_like(p) for p in params]
    else:
        raise KeyError(kind)
    out = []
    for t, (flat_g, lr) in enumerate(zip(grads, lrs), start=1):
        for p, g in zip(params, _split(entries, flat_g, dtype)):
            p.grad = g * grad_scale
        if max_norm > 0:
            norm = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
        else:
            norm = math.sqrt(sum(float(p.grad.double().pow(2).sum()) for p in params))
        if opt is not None:
            for g in opt.param_groups:
                g["lr"] = lr
            opt.step()
            if kind == "sgd":
                state = {"momentum_buffer": [opt.state[p].get("momentum_buffer") for p in params]}
                if hp["momentum"] == 0:
                    state = {}
            else:
                state = {"exp_avg": [opt.state[p]["exp_avg"] for p in params],
                         "exp_avg_sq": [opt.state[p]["exp_avg_sq"] for p in params]}
        else:
            _lamb_step(params, entries, m, v, t, lr, hp, wd)
            state = {"exp_avg": m, "exp_avg_sq": v}
        out.append({"params": [p.detach().clone() for p in params],
                    "state": {k: [s.detach().clone() for s in ts] for k, ts in state.items()},
                    "norm": norm})
    return out


@torch.no_grad()
def _lamb_step(params, entries, m, v, t, lr, hp, wd) -> None:
    b1, b2 = hp["betas"]
    eps = hp["eps"]
    bias = bool(hp.get("bias_correction", True))
    bc1 = 1 - b1 ** t if bias else 1.0
    bc2 = 1 - b2 ** t if bias else 1.0
    for p, e, mi, vi in zip(params, entries, m, v):
        g = p.grad
        mi.mul_(b1).add_(g, alpha=1 - b1)
        vi.mul_(b2).add_(g * g, alpha=1 - b2)
        u = (mi / bc1) / ((vi / bc2).sqrt() + eps)
        if e.decay and wd:
            u = u + wd * p
        pn, un = float(torch.linalg.vector_norm(p)), float(torch.linalg.vector_norm(u))
        ratio = pn / un if pn > 0 and un > 0 else 1.0
        p.sub_(u * (lr * ratio))


def flatten(entries, tensors: Sequence[torch.Tensor], numel: int) -> torch.Tensor:
    """Per-tensor float64 results laid out as the arena is (pads zero)."""
    out = torch.zeros(numel, dtype=torch.float64)
    for e, t in zip(entries, tensors):
        out[e.offset:e.offset + e.numel] = t.reshape(-1).double()
    return out


def ulp32(x: float) -> float:
    """The spacing of fp32 numbers at ``|x|``."""
    t = torch.tensor(abs(float(x)), dtype=torch.float32)
    return float(torch.nextafter(t, torch.tensor(float("inf"))).double() - t.double())


def bound(o64: torch.Tensor, o32: torch.Tensor):
    """(yard, tolerance) for one quantity: ``yard = max|oracle_fp32 - oracle_fp64|`` on the same
    inputs, tolerance ``MARGIN * yard + ulp32(max|oracle_fp64|)``.  The margin covers what a
    kernel may do differently from ``torch.optim`` in fp32, each worth about one more rounding:
    decay folded into a multiply, ``lr/bc1`` and ``rsqrt(bc2)`` computed once, FMA contraction,
    atomic-order norms in LAMB."""
    yard = float((o32.double() - o64).abs().max())
    return yard, MARGIN * yard + ulp32(float(o64.abs().max()))


# ---------------------------------------------------------------------------- the fixture
# (name, shape): ``default_no_decay`` gives both kinds, by rank and by name.
TENSORS = [
    ("head.bias", (5,)),            # zero-initialised: LAMB's ||p|| == 0 branch on step 1
    ("ln.weight", (129,)),
    ("fc1.weight", (64, 128)),      # exactly one 8192-element table row
    ("emb.bias", (8193,)),          # a second row of length 8 that holds 1 real element
    ("fc2.weight", (67, 129)),      # 8643
    ("big.weight", (136, 181)),     # 24616 = 3 * 8192 + 40: four rows feed one LAMB norm slot
    ("norm.weight", (3, 7)),        # 2-D but no decay (by name); its gradient is always zero
]
ZERO_INIT = "head.bias"
ZERO_GRAD = "norm.weight"
STEPS = 5
GRAD_SCALE = 0.5
GRAD_STD = 0.005          # ||g|| * GRAD_SCALE is ~0.56 on ordinary steps and ~5.6 on step 2
BIG_STEP = 1              # (0-based) the step whose gradient is 10x larger
LR_CHANGE_STEP = 3        # (0-based) the step handed a new lr through step(lr=...)


def make_params(dtype, device, integers: bool = False) -> List:
    """Fresh bare parameters (the arena rebinds ``.data``, so every case builds its own)."""
    g = torch.Generator().manual_seed(11)
    out = []
    for name, shape in TENSORS:
        if integers:
            t = torch.randint(-4, 5, shape, generator=g).float()
        else:
            t = torch.randn(shape, generator=g) * 0.5
        if name == ZERO_INIT:
            t.zero_()
        out.append((name, torch.nn.Parameter(t.to(dtype).to(device))))
    return out


def pad_mask(arena) -> torch.Tensor:
    """True on the alignment pads of the arena (CPU bool)."""
    m = torch.ones(arena.numel, dtype=torch.bool)
    for e in arena.entries:
        m[e.offset:e.offset + e.numel] = False
    return m


def make_grads(arena, dtype, steps: int = STEPS, integers: bool = False) -> List[torch.Tensor]:
    """Per-step flat CPU gradients in ``dtype``: zero in the pads and on ``ZERO_GRAD``; step
    ``BIG_STEP`` is 10x larger so that a clip at 1.0 binds on it and not on the others."""
    g = torch.Generator().manual_seed(23)
    live = ~pad_mask(arena)
    for e in arena.entries:
        if e.name == ZERO_GRAD:
            live[e.offset:e.offset + e.numel] = False
    out = []
    for s in range(steps):
        if integers:
            t = torch.randint(-4, 5, (arena.numel,), generator=g).float()
        else:
            t = torch.randn(arena.numel, generator=g) * (GRAD_STD * (10.0 if s == BIG_STEP else 1.0))
        out.append((t * live).to(dtype))
    return out


def make_lrs(lr: float, steps: int = STEPS) -> List[float]:
    return [lr if s < LR_CHANGE_STEP else lr * 0.5 for s in range(steps)]


def default_hp(kind: str, **over) -> Dict[str, object]:
    hp = {"sgd": dict(lr=0.1, momentum=0.9, nesterov=False, weight_decay=0.1, max_grad_norm=0.0),
          "adamw": dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.1, max_grad_norm=0.0),
          "lamb": dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.1, max_grad_norm=0.0,
                       bias_correction=True)}[kind]
    hp.update(over)
    return hp


_ORACLE_CACHE: Dict[object, object] = {}


def oracle_pair(kind, arena, init, grads, hp, lrs, grad_scale, key: Optional[object] = None):
    """(float64 run, float32 run) of the oracle, computed once per ``key`` and left unchanged."""
    if key is not None and key in _ORACLE_CACHE:
        return _ORACLE_CACHE[key]
    pair = tuple(run_oracle(kind, arena.entries, init, grads, hp, lrs, grad_scale, dtype=dt)
                 for dt in (torch.float64, torch.float32))
    if key is not None:
        _ORACLE_CACHE[key] = pair
    return pair


# ---------------------------------------------------------------------------- flat optimizer vs oracle
# Only this section touches the code under test; the oracle above never does.
def make_arena(device, pdtype, shard: bool = False, integers: bool = False):
    from databricks_distributed_deep_learning_amd.optim import ParamArena
    return ParamArena(make_params(pdtype, device, integers), pad_multiple=128 if shard else 1)


def make_opt(kind: str, arena, hp, shard: bool = False):
    """ZeRO-1 (``shard``): rank 0 of 2 owning chunk 0 of two buckets; the collectives are stubbed
    by the caller (``_sum_over_ranks``) and here (``gather_fn``)."""
    from databricks_distributed_deep_learning_amd.optim import FlatAdamW, FlatLAMB, FlatSGD
    spec = None
    if shard:
        split = (arena.numel // 2) // 128 * 128
        spec = (0, 2, [(0, split), (split, arena.numel)])
    common = dict(lr=hp["lr"], weight_decay=hp["weight_decay"], max_grad_norm=hp["max_grad_norm"], shard=spec)
    if kind == "sgd":
        opt = FlatSGD(arena, momentum=hp["momentum"], nesterov=hp["nesterov"], **common)
    elif kind == "adamw":
        opt = FlatAdamW(arena, betas=hp["betas"], eps=hp["eps"], **common)
    else:
        opt = FlatLAMB(arena, betas=hp["betas"], eps=hp["eps"], bias_correction=hp["bias_correction"], **common)
    if shard:
        opt.gather_fn = lambda groups, ranges: None
    return opt


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).cpu()


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def snapshot(opt, arena) -> Dict[str, torch.Tensor]:
    snap = {"master": opt.params32.detach().clone(), "flat": arena.flat.detach().clone()}
    snap.update({k: v.detach().clone() for k, v in opt._state_tensors().items()})
    return snap


def range_bounds(arena) -> List:
    """Three tensor-aligned ranges covering the arena (as a bucketed reducer hands them over)."""
    a, b = arena.entries[2].offset, arena.entries[5].offset
    return [(0, a), (a, b), (b, arena.numel)]


class FlatRun:
    """One flat optimizer on the fixture, stepped beside the oracle and checked after every step.

    ``ratios`` collects, per quantity, the worst ``max|flat - oracle_fp64| / yard`` seen."""

    def __init__(self, kind, device, pdtype, gdtype, hp, *, shard=False, integers=False, steps=STEPS,
                 exact=False, nan_buffer=False):
        self.kind, self.device, self.pdtype, self.gdtype, self.hp = kind, device, pdtype, gdtype, dict(hp)
        self.shard, self.integers, self.steps, self.exact = shard, integers, steps, exact
        self.arena = make_arena(device, pdtype, shard, integers)
        self.opt = make_opt(kind, self.arena, hp, shard)
        self.grads = make_grads(self.arena, gdtype, steps, integers)
        self.lrs = make_lrs(hp["lr"], steps)
        init = self.arena.flat.detach().cpu()
        key = (kind, pdtype, gdtype, tuple(sorted(hp.items())), shard, integers, steps)
        self.o64, self.o32 = oracle_pair(kind, self.arena, init, self.grads, hp, self.lrs, GRAD_SCALE, key)
        # local index -> arena index of the owned elements
        self.sel = torch.cat([torch.arange(lo, hi) for lo, hi, _ in self.opt.ranges])
        self.pads = pad_mask(self.arena)
        self.before = self.arena.flat.detach().clone()
        self.nan_buffer = nan_buffer
        if nan_buffer:
            self.opt.buf.fill_(float("nan"))
            self.buf0 = self.opt.buf.clone()
        self.ratios: Dict[str, float] = {}
        self.snaps: List[Dict[str, torch.Tensor]] = []
        self.done = 0

    # -- stepping
    def _local(self, g: torch.Tensor) -> torch.Tensor:
        return g if not self.shard else torch.cat([g[lo:hi] for lo, hi, _ in self.opt.ranges])

    def step(self, ranges: bool = False, check: bool = True) -> None:
        s = self.done
        g = self.grads[s].to(self.device)
        lr = self.lrs[s] if s == LR_CHANGE_STEP else None
        if ranges:
            self.opt.begin_step(lr)
            for lo, hi in reversed(range_bounds(self.arena)):
                self.opt.step_range(g, GRAD_SCALE, lo, hi)
            self.opt.end_step()
        else:
            self.opt.step(self._local(g), grad_scale=GRAD_SCALE, lr=lr)
        self.done += 1
        self.snaps.append(snapshot(self.opt, self.arena))
        if check:
            self.check(s)

    def run(self, ranges: bool = False, resume_at: Optional[int] = None) -> "FlatRun":
        while self.done < self.steps:
            if resume_at is not None and self.done == resume_at:
                self.resume()
            self.step(ranges)
        return self

    def resume(self) -> None:
        """Checkpoint, then go on with a FRESH arena and optimizer restored from it: the model's
        parameters as a model checkpoint restores them, the rest through ``load_state_dict``."""
        st = {k: (v.detach().clone() if isinstance(v, torch.Tensor) else v) for k, v in self.opt.state_dict().items()}
        flat = self.arena.flat.detach().clone()
        self.arena = make_arena(self.device, self.pdtype, self.shard, self.integers)
        self.opt = make_opt(self.kind, self.arena, self.hp, self.shard)
        self.arena.flat.copy_(flat)
        self.opt.load_state_dict(st)

    # -- checking
    def check(self, s: int) -> None:
        opt, arena, sel = self.opt, self.arena, self.sel
        o64, o32 = self.o64[s], self.o32[s]
        what = f"{self.kind} {self.pdtype}/{self.gdtype} step {s + 1}"
        quantities = {"master": (opt.params32, o64["params"], o32["params"])}
        for k, t in opt._state_tensors().items():
            if k in o64["state"]:
                quantities[k] = (t, o64["state"][k], o32["state"][k])
        for name, (t, r64, r32) in quantities.items():
            f64 = flatten(arena.entries, r64, arena.numel)[sel]
            f32 = flatten(arena.entries, r32, arena.numel)[sel]
            got = t.detach().cpu().double()
            assert got.shape == f64.shape, f"{what} {name}: {tuple(got.shape)} elements, expected {tuple(f64.shape)}"
            err = float((got - f64).abs().max())
            if self.exact:
                assert torch.equal(f32, f64), f"{what} {name}: the fp32 oracle is not exact on these inputs"
                assert err == 0.0, f"{what} {name}: differs from the exact result by {err:.3e}"
                continue
            yard, tol = bound(f64, f32)
            ratio = err / yard if yard > 0 else (0.0 if err == 0 else float("inf"))
            self.ratios[name] = max(self.ratios.get(name, 0.0), ratio)
            assert err <= tol, (f"{what} {name}: max|flat - oracle64| = {err:.3e} > {tol:.3e} "
                                f"(yard {yard:.3e}, error/yard = {ratio:.2f}, margin {MARGIN})")
        # the compute-dtype copy is the rounded master, written in the same pass
        if arena.dtype == torch.bfloat16:
            want = opt.params32.detach().to(torch.bfloat16)
            assert same_bits(arena.flat[sel.to(arena.flat.device)], want), f"{what}: bf16 copy != RNE(master)"
        elif not self.shard:
            assert opt.params32 is arena.flat
        # alignment pads stay exactly zero, in the arena and in every local tensor
        lpads = self.pads[sel]
        assert not bool(arena.flat.detach().cpu()[self.pads].any()), f"{what}: arena pad written"
        for name, t in [("master", opt.params32)] + list(opt._state_tensors().items()):
            if self.nan_buffer and name == "momentum_buffer":
                continue
            assert not bool(t.detach().cpu()[lpads].any()), f"{what}: {name} pad written"
        if self.nan_buffer:     # momentum 0: the buffer is neither read nor written
            assert same_bits(opt.buf, self.buf0), f"{what}: momentum buffer touched with momentum=0"
        if self.shard:          # another rank's elements are left to the (stubbed) all-gather
            owned = torch.zeros(arena.numel, dtype=torch.bool)
            owned[sel] = True
            assert same_bits(arena.flat.detach().cpu()[~owned], self.before.cpu()[~owned]), f"{what}: unowned written"

    def clip_activity(self):
        """(steps on which the clip binds, steps on which it does not), from the oracle's norms."""
        mx = float(self.hp["max_grad_norm"])
        act = [mx / (o["norm"] + 1e-6) < 1.0 for o in self.o64]
        return sum(act), len(act) - sum(act)

    def report(self) -> str:
        return "ORACLE-RATIO %s %s" % (self.kind, " ".join(f"{k}={v:.3f}" for k, v in sorted(self.ratios.items())))
