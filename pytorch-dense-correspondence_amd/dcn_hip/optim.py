"""`optimizer.step()` of the training step as one HIP pass (dcn_adam_step, csrc/optim_kernels.hip).

The reference builds `torch.optim.Adam(dcn.parameters(), lr=1e-4, weight_decay=1e-4)` (training.py:133-145) and
calls `optimizer.zero_grad()` / `optimizer.step()` every iteration (training.py:325,346); `adjust_learning_rate`
(training.py:544-558) rewrites `param_group['lr']`, `save_network` (training.py:501-521) stores
`optimizer.state_dict()`.  `Adam` below has the same constructor, the same per-parameter state (`step`, `exp_avg`,
`exp_avg_sq`) and therefore the same `state_dict()` layout -- a `.pth.opt` file of either class loads into the other --
but updates all parameters of a group with one kernel launch per 80 tensors instead of ~10 passes over the 85 MB of
parameters.  There is no CPU fallback: without the HIP library `step()` raises.

`GuardedAdam` is the same update with the step count, the learning rate and the bias corrections kept on the device
(dcn_adam_step_guarded, csrc/train_kernels.hip), for a training loop that decides there whether an iteration counts
(dcn_hip.train)."""
import ctypes

import torch

from . import _lib


def _dense(t):
    """True when the tensor's elements occupy numel() consecutive floats in SOME dimension order."""
    dims = sorted((d for d in range(t.dim()) if t.shape[d] != 1), key=lambda d: t.stride(d))
    expect = 1
    for d in dims:
        if t.stride(d) != expect:
            return False
        expect *= t.shape[d]
    return True


def _like_param(t, p):
    """`t` with the memory order of the parameter `p` (element k of the storage of both is the same logical element)."""
    if t.stride() == p.stride() and t.dtype == p.dtype and t.device == p.device:
        return t
    out = torch.empty_like(p, memory_format=torch.preserve_format)
    if out.stride() != p.stride():  # preserve_format keeps the strides of a dense tensor; anything else is unsupported
        raise ValueError("dcn_hip.optim.Adam: cannot lay out optimizer state like a parameter with strides %s" % (p.stride(),))
    out.copy_(t)
    return out


class Adam(torch.optim.Optimizer):
    """torch.optim.Adam semantics (L2 weight decay added to the gradient, bias correction, no amsgrad) for dense fp32
    parameters on the GPU."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False):
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {}".format(eps))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter at index 0: {}".format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter at index 1: {}".format(betas[1]))
        if not 0.0 <= weight_decay:
            raise ValueError("Invalid weight_decay value: {}".format(weight_decay))
        if amsgrad:
            raise NotImplementedError("dcn_hip.optim.Adam: amsgrad is not implemented (the reference does not use it)")
        super(Adam, self).__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False,
                                                maximize=False))

    def zero_grad(self, set_to_none=True):
        """``optimizer.zero_grad()`` of training.py:325.  When the gradients are views of a flat buffer
        (``dcn_hip.distributed.FlatGradients(...).attach(optimizer)``) they are zeroed IN PLACE with one kernel whatever
        ``set_to_none`` says -- dropping the views would detach ``p.grad`` from the buffer the collective averages."""
        flat = getattr(self, "_flat_gradients", None)
        if flat is not None:
            flat.zero_()
            return
        super(Adam, self).zero_grad(set_to_none=set_to_none)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.get()
        for gi, group in enumerate(self.param_groups):
            if group.get("amsgrad") or group.get("maximize"):
                raise NotImplementedError("dcn_hip.optim.Adam: amsgrad / maximize are not implemented")
            if self._fast_step(lib, gi, group):
                continue
            by_step = {}
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse:
                    raise RuntimeError("Adam does not support sparse gradients, please consider SparseAdam instead")
                if p.dtype != torch.float32 or g.dtype != torch.float32:
                    raise TypeError("dcn_hip.optim.Adam: float32 parameters and gradients only")
                if not _dense(p):
                    raise ValueError("dcn_hip.optim.Adam: parameter storage must be dense, got strides %s" % (p.stride(),))
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                # state loaded from a checkpoint written with another memory format: re-lay it once
                st["exp_avg"] = _like_param(st["exp_avg"], p)
                st["exp_avg_sq"] = _like_param(st["exp_avg_sq"], p)
                g = _like_param(g, p)
                _lib.require_device(p, g, st["exp_avg"], st["exp_avg_sq"])
                if not torch.is_tensor(st["step"]):
                    st["step"] = torch.tensor(float(st["step"]), dtype=torch.float32)
                st["step"] += 1
                by_step.setdefault(int(st["step"].item()), []).append((p, g, st["exp_avg"], st["exp_avg_sq"]))
            beta1, beta2 = group["betas"]
            for t, items in by_step.items():
                n = len(items)
                cols = [(ctypes.c_void_p * n)(*[x[k].data_ptr() for x in items]) for k in range(4)]
                numel = (ctypes.c_int64 * n)(*[x[0].numel() for x in items])
                rc = lib.dcn_adam_step(n, cols[0], cols[1], cols[2], cols[3], numel, float(group["lr"]), float(beta1),
                                       float(beta2), float(group["eps"]), float(group["weight_decay"]), t,
                                       _lib.stream_ptr())
                _lib.check(rc, "dcn_adam_step")
            if len(by_step) == 1:   # every parameter of the group at the same step: the next call can take the fast path
                (t, items), = by_step.items()
                if len(items) == len(group["params"]):
                    self._fast = getattr(self, "_fast", {})
                    # (pointers and shapes only for the gradients: the cache must not keep last step's gradient tensors alive)
                    self._fast[gi] = {"t": t, "items": [(it[0], None, it[2], it[3]) for it in items], "cols": cols,
                                      "numel": numel, "ptrs": [tuple(x.data_ptr() for x in it) for it in items],
                                      "steps": [self.state[it[0]]["step"] for it in items]}
        return loss

    def _fast_step(self, lib, gi, group):
        """The steady state of a training loop -- the same parameters, gradient buffers and state tensors as in the previous
        call, all at the same step: one launch from the pointer tables of the previous call, after checking that nothing moved
        (110 parameters x the per-parameter checks, state-dict lookups and .item() of the general path were ~2 ms of host time
        per step: what bounds the reference's batch size of 1 is the host).  Anything unexpected: the general path."""
        fast = getattr(self, "_fast", {}).get(gi)
        if fast is None:
            return False
        params = group["params"]
        items = fast["items"]
        if len(params) != len(items):
            self._fast.pop(gi, None)
            return False
        for p, it, ptr, st in zip(params, items, fast["ptrs"], fast["steps"]):
            g = p.grad
            state = self.state.get(p)
            # (pointer, strides and dtype of the gradient are compared on EVERY call: the same tensor object may have been
            # re-pointed -- `p.grad.data = ...`, `set_`, a bucket view reassigned -- and the cached tables hold addresses)
            if (p is not it[0] or g is None or g.data_ptr() != ptr[1] or g.stride() != p.stride() or g.dtype != p.dtype
                    or g.is_sparse or state is None or state.get("exp_avg") is not it[2] or state.get("exp_avg_sq") is not it[3]
                    or it[2].data_ptr() != ptr[2] or it[3].data_ptr() != ptr[3]
                    or state.get("step") is not st or p.data_ptr() != ptr[0]):
                self._fast.pop(gi, None)
                return False
        t = fast["t"] + 1
        torch._foreach_add_(fast["steps"], 1.0)    # the per-parameter step counters (host tensors), one call
        beta1, beta2 = group["betas"]
        cols = fast["cols"]
        rc = lib.dcn_adam_step(len(items), cols[0], cols[1], cols[2], cols[3], fast["numel"], float(group["lr"]), float(beta1),
                               float(beta2), float(group["eps"]), float(group["weight_decay"]), t, _lib.stream_ptr())
        _lib.check(rc, "dcn_adam_step")
        fast["t"] = t
        return True


class GuardedAdam(Adam):
    """``Adam`` whose step count, learning rate and bias corrections live in a device-resident training state
    (``dcn_hip.train.TrainState``, struct dcn_train_state) and whose update is skipped ON THE DEVICE when that state says the
    iteration does not count (dcn_adam_step_guarded, csrc/train_kernels.hip) -- the reference's ``continue`` on an empty
    sample (training.py:304-306) without a host read.

    Same constructor and ``state_dict()`` layout as ``Adam``: checkpoints interchange with ``Adam`` and ``torch.optim.Adam``.
    ``step(state)`` launches the guarded kernel and leaves the host-side per-parameter ``step`` tensors alone; ``state_dict()``
    reads ``t`` and ``lr`` from the device once, fills every parameter's ``step`` and ``param_groups[0]['lr']`` with them;
    ``load_state_dict`` seeds the device ``t`` and ``lr`` (all loaded steps must be equal: there is one count on the device).
    One parameter group; every parameter needs a gradient in every step."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False):
        super(GuardedAdam, self).__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad)
        if len(self.param_groups) != 1:
            raise ValueError("dcn_hip.optim.GuardedAdam: one parameter group only (the device state holds one step count "
                             "and one learning rate), got %d" % len(self.param_groups))
        self._train_state = None

    def add_param_group(self, param_group):
        if len(self.param_groups) >= 1:
            raise ValueError("dcn_hip.optim.GuardedAdam: one parameter group only")
        super(GuardedAdam, self).add_param_group(param_group)

    # ---- the device state
    def _common_step(self):
        """The step count all parameters with state share (0 without state); raises when they differ."""
        steps = set()
        for p in self.param_groups[0]["params"]:
            st = self.state.get(p)
            if st:
                steps.add(float(st["step"]))
        if len(steps) > 1:
            raise ValueError("dcn_hip.optim.GuardedAdam: the per-parameter steps differ (%s): the device state holds ONE step "
                             "count" % sorted(steps)[:4])
        t = steps.pop() if steps else 0.0
        if t != int(t) or t < 0:
            raise ValueError("dcn_hip.optim.GuardedAdam: step %r is not a count" % t)
        return int(t)

    def bind(self, state, seed=True):
        """Make ``state`` (a ``dcn_hip.train.TrainState``) this optimizer's state block.  ``seed``: its ``t`` and ``lr`` are set
        from the host-side steps and ``param_groups[0]['lr']`` (a start, or a checkpoint just loaded).  ``step(state)`` with a
        state that was never bound adopts it as it is -- ``advance`` has already counted the step by then."""
        betas = tuple(float(b) for b in self.param_groups[0]["betas"])
        if tuple(float(b) for b in state.betas) != betas:
            raise ValueError("dcn_hip.optim.GuardedAdam: the training state computes the bias corrections with betas %s, the "
                             "optimizer has %s" % (tuple(state.betas), betas))
        if seed:
            state.seed(self._common_step(), float(self.param_groups[0]["lr"]))
        self._train_state = state
        return state

    def state_dict(self, known=None):
        """``known``: (t, lr) already read from the device by the caller (``TrainState.read()``), to save the read here."""
        if self._train_state is not None:
            t, lr = known if known is not None else self._train_state.read_step_and_lr()
            for p in self.param_groups[0]["params"]:
                st = self.state.get(p)
                if st:
                    st["step"] = torch.tensor(float(t), dtype=torch.float32)
            self.param_groups[0]["lr"] = float(lr)
        return super(GuardedAdam, self).state_dict()

    def load_state_dict(self, state_dict):
        if len(state_dict["param_groups"]) != 1:
            raise ValueError("dcn_hip.optim.GuardedAdam: one parameter group only, the checkpoint has %d"
                             % len(state_dict["param_groups"]))
        steps = set(float(s["step"]) for s in state_dict["state"].values() if "step" in s)
        if len(steps) > 1:
            raise ValueError("dcn_hip.optim.GuardedAdam: the loaded per-parameter steps differ (%s): the device state holds "
                             "ONE step count" % sorted(steps)[:4])
        super(GuardedAdam, self).load_state_dict(state_dict)
        if self._train_state is not None:
            self.bind(self._train_state)

    @torch.no_grad()
    def step(self, state=None, closure=None):
        if state is None or not hasattr(state, "state_ptr"):
            raise TypeError("dcn_hip.optim.GuardedAdam.step(state): the device-resident training state "
                            "(dcn_hip.train.TrainState) decides whether and with which scalars the update runs")
        if closure is not None:
            raise NotImplementedError("dcn_hip.optim.GuardedAdam: no closure (the loss is not re-evaluated)")
        if len(self.param_groups) != 1:
            raise ValueError("dcn_hip.optim.GuardedAdam: one parameter group only")
        group = self.param_groups[0]
        if group.get("amsgrad") or group.get("maximize"):
            raise NotImplementedError("dcn_hip.optim.GuardedAdam: amsgrad / maximize are not implemented")
        if self._train_state is not state:
            self.bind(state, seed=False)
        params = group["params"]
        n = len(params)
        cols = [(ctypes.c_void_p * n)() for _ in range(4)]
        numel = (ctypes.c_int64 * n)()
        keep = []                               # gradients re-laid like their parameter: alive until the launch is enqueued
        for i, p in enumerate(params):
            g = p.grad
            if g is None:
                raise RuntimeError("dcn_hip.optim.GuardedAdam: parameter %d has no gradient; the device state holds one step "
                                   "count for all parameters, so every one of them takes part in every step" % i)
            if g.is_sparse:
                raise RuntimeError("Adam does not support sparse gradients, please consider SparseAdam instead")
            st = self.state[p]
            if len(st) == 0 or st["exp_avg"].stride() != p.stride() or st["exp_avg_sq"].stride() != p.stride() \
                    or g.stride() != p.stride() or g.dtype != torch.float32:
                if p.dtype != torch.float32 or g.dtype != torch.float32:
                    raise TypeError("dcn_hip.optim.GuardedAdam: float32 parameters and gradients only")
                if not _dense(p):
                    raise ValueError("dcn_hip.optim.GuardedAdam: parameter storage must be dense, got strides %s" % (p.stride(),))
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg"] = _like_param(st["exp_avg"], p)
                st["exp_avg_sq"] = _like_param(st["exp_avg_sq"], p)
                g = _like_param(g, p)
                keep.append(g)
            _lib.require_device(p, g, st["exp_avg"], st["exp_avg_sq"])
            cols[0][i], cols[1][i] = p.data_ptr(), g.data_ptr()
            cols[2][i], cols[3][i] = st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
            numel[i] = p.numel()
        beta1, beta2 = group["betas"]
        rc = _lib.get().dcn_adam_step_guarded(n, cols[0], cols[1], cols[2], cols[3], numel, float(group["eps"]),
                                              float(group["weight_decay"]), float(beta1), float(beta2),
                                              ctypes.c_void_p(state.state_ptr()), _lib.stream_ptr())
        _lib.check(rc, "dcn_adam_step_guarded")
        return None
