"""SGD with momentum as ONE multi-tensor HIP launch per step (reference: optim.SGD at train.py:196); ``Adam`` and the
parameter moving average ``ParamEMA`` on the same table / chunk scheme.

Same constructor shape as ``torch.optim.SGD`` (param groups with per-group ``weight_decay`` / ``lr``), same
update:  d = g + wd*p ; buf = momentum*buf + d ; p -= lr*buf, with buf starting at zero so
the first step yields buf = d.  Parameters whose ``.grad`` is None (frozen body, train.py:263-268) are
skipped entirely.  ``param_groups`` stay plain dicts so warm_up_lr / schedule_lr work unchanged.

A parameter that carries ``_frhip_row_grad = (idx, rows)`` (the sampled class-sharded head with ``sparse_update=True``,
frhip/sharded_head.py) takes the same update on the rows ``idx`` alone, in one launch of its own (fr_sgd_rows): the lazy
update of Partial-FC v1, where an unselected row sees no weight decay and no momentum step.  ``SGD`` only; ``Adam`` refuses.

``GradGuard`` measures the global L2 norm of a parameter set's gradients on the device (two small launches) and leaves a
control word there -- norm, clip coefficient, go flag -- that ``SGD.step(guard=...)`` / ``Adam.step(guard=...)`` consume:
global-norm clipping and the skip of a step whose gradients are not finite, with no host read and no second pass over the
gradients.  Without a guard the optimizers run exactly the launches they ran before it existed.
"""
import ctypes
import itertools

import torch

from . import _lib, ops


class SGD(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0, weight_decay=0.0, nesterov=False, *,
                 maximize=False):
        # the defaults carry every key torch.optim.SGD reads in step(): an Optimizer_*.pth written here loads into
        # the reference's torch.optim.SGD (train.py:196, :227-230) and steps there, and the other way round
        if dampening != 0 or nesterov or maximize:
            raise NotImplementedError("frhip.optim.SGD implements the reference's update only (train.py:196: dampening 0, "
                                      "no nesterov, minimise)")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                      nesterov=nesterov, maximize=maximize, foreach=None, differentiable=False,
                                      fused=None))
        self._sig = None
        self._tables = []  # per group: [(table_dev, chunks_dev, nchunks, use_coef)], one entry without a guard

    def zero_grad(self, set_to_none=False):
        """Keeps gradient buffers alive (the engine writes into them).  Gradients that are views of an engine
        gradient arena are cleared with ONE fill of the arena instead of one launch per parameter.
        (Round 6, measured and taken back: dropping the gradients that are not arena views -- the head's -- so that autograd
        installs the new tensor instead of adding it onto zeros saves a fill and an add of N x 512 floats per step, 14 us at
        7000 classes; but the optimizer's launch tables are keyed on the gradient addresses, and a step whose allocator hands
        out another block rebuilds them: not worth the exposure.)"""
        arenas = {}
        for group in self.param_groups:
            for p in group["params"]:
                g = p.grad
                if getattr(p, "_frhip_row_grad", None) is not None:  # a row gradient nobody consumed (sharded_head.py)
                    p._frhip_row_grad = None
                if g is None:
                    continue
                if set_to_none:
                    p.grad = None
                elif g._is_view() and getattr(g._base, "_frhip_grad_arena", False):
                    arenas[id(g._base)] = g._base
                else:
                    g.zero_()
        for a in arenas.values():
            a.zero_()
            a._frhip_zeroed = True  # the engine's next backward skips its own fill (engine.run_backward)

    def _build(self, guard=None):
        """Per group the launch tables [(table_dev, chunks_dev, nchunks, use_coef)]: one table without a guard; with one,
        the tensors of the guard's parameter set (use_coef 1: clipped) apart from the rest (use_coef 0: go flag only)."""
        for group in self.param_groups:  # a loaded state dict may carry settings this kernel does not implement
            if group.get("dampening", 0) != 0 or group.get("nesterov", False) or group.get("maximize", False):
                raise NotImplementedError("frhip.optim.SGD: dampening / nesterov / maximize are not implemented")
        chunk = _lib.lib.fr_sgd_chunk_elems()
        self._tables = []
        for group in self.param_groups:
            split = {}  # use_coef -> (records, chunks)
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not p.is_cuda:
                    raise _lib.FrhipError("frhip.optim.SGD: parameter on %s -- the HIP optimizer needs ROCm tensors"
                                          % p.device)
                st = self.state[p]
                if "momentum_buffer" not in st:
                    st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                buf, g = st["momentum_buffer"], p.grad
                if buf is None:  # torch.optim.SGD writes None before its first step
                    buf = st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                if buf.shape == p.shape and not _dense_same(p, buf):
                    # a buffer loaded from a checkpoint written with another memory layout (the reference's
                    # torch.optim.SGD keeps OIHW-contiguous buffers; the conv weights here are channels-last)
                    relaid = torch.empty_like(p, memory_format=torch.preserve_format)
                    relaid.copy_(buf)
                    buf = st["momentum_buffer"] = relaid
                if not (_dense_same(p, g) and _dense_same(p, buf)):
                    raise _lib.FrhipError("frhip.optim.SGD: param / grad / momentum buffer must share one dense layout")
                n = p.numel()
                recs, chunks = split.setdefault(1 if guard is not None and guard.covers(p) else 0, ([], []))
                t = len(recs)
                recs.append((p.data_ptr(), g.data_ptr(), buf.data_ptr(), n, float(group["weight_decay"])))
                chunks.extend((t, c) for c in range((n + chunk - 1) // chunk))
            if not split:
                self._tables.append(None)
                continue
            tabs = []
            for use_coef, (recs, chunks) in split.items():
                arr = (_lib.FrSgdTensor * len(recs))()
                for i, (pp, gp, bp, n, wd) in enumerate(recs):
                    arr[i].p, arr[i].g, arr[i].buf, arr[i].n, arr[i].wd = pp, gp, bp, n, wd
                dev = group["params"][0].device
                raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
                ch = torch.tensor(chunks, dtype=torch.int32).reshape(-1).to(dev)
                tabs.append((raw, ch, len(chunks), use_coef))
            self._tables.append(tabs)

    def load_state_dict(self, state_dict):
        """As torch.optim.Optimizer.load_state_dict (works before the first step, like the reference's resume at
        train.py:227-230); the launch tables are rebuilt because the momentum buffers are new tensors."""
        super().load_state_dict(state_dict)
        self._sig = None

    def _signature(self):
        return tuple((p.data_ptr(), 0 if p.grad is None else p.grad.data_ptr(), float(g["weight_decay"]))
                     for g in self.param_groups for p in g["params"])

    @torch.no_grad()
    def step(self, closure=None, guard=None):
        """One update.  ``guard``: a ``GradGuard`` whose ``measure()`` ran for this step.  The update then goes through the
        ``_ctl`` entry points: nothing moves when the guard's go flag is 0; the tensors of the guard's parameter set take
        their gradient times the clip coefficient, the rest (the head) take it as it is and obey the go flag only -- at most
        one launch more per parameter group; a row gradient goes through fr_sgd_rows_ctl.  ``.grad`` is never modified: the
        coefficient is applied where the gradient is read (torch's ``clip_grad_norm_`` scales ``.grad`` in place; code that
        reads ``.grad`` after the step sees the unclipped values here).  Without a guard: the launches of before."""
        loss = closure() if closure is not None else None
        ctl = guard._take("frhip.optim.SGD") if guard is not None else None
        # parameters that carry a row gradient (sharded_head.py, sparse_update): their .grad is None, so the dense tables
        # leave them out and the signature does not move with them
        rows = _row_grad_params(self.param_groups)
        for _group, p in rows:
            if p.grad is not None:
                raise _lib.FrhipError("frhip.optim.SGD: a parameter carries a row gradient (sparse_update) and a dense "
                                      ".grad; the two cannot be combined -- set the dense one to None")
        sig = (self._signature(), None if guard is None else guard.key)
        if sig != self._sig:
            if guard is None:
                self._build()
            else:
                self._build(guard)
            self._sig = sig
        st = ops.current_stream_ptr()
        for group, tabs in zip(self.param_groups, self._tables):
            for raw, ch, n, use_coef in tabs or ():
                table = ctypes.cast(ctypes.c_void_p(raw.data_ptr()), ctypes.POINTER(_lib.FrSgdTensor))  # device array
                if ctl is None:
                    ops.Launch("fr_sgd_step", [table, ctypes.c_void_p(ch.data_ptr()), n, float(group["lr"]),
                                               float(group["momentum"]), st])()
                else:
                    ops.Launch("fr_sgd_step_ctl", [table, ctypes.c_void_p(ch.data_ptr()), n, float(group["lr"]),
                                                   float(group["momentum"]), ops.ptr(ctl), use_coef, st])()
        for group, p in rows:
            self._step_rows(group, p, st, ctl)
        return loss

    def _step_rows(self, group, p, st, ctl=None):
        """The lazy update of Partial-FC v1 on a parameter that carries ``_frhip_row_grad = (idx, rows)`` (a sampled
        ``ShardedMarginLoss(sparse_update=True)``): d = rows[j] + wd p[r]; buf[r] = momentum buf[r] + d; p[r] -= lr buf[r]
        on the rows r = idx[j] of the parameter and of its momentum buffer in one launch (fr_sgd_rows: the expression of the
        dense step, the same roundings).  The other rows keep their bits: no weight decay, no momentum step.  The momentum
        buffer is the dense tensor the dense path keeps, so state dicts do not change."""
        if group.get("dampening", 0) != 0 or group.get("nesterov", False) or group.get("maximize", False):
            raise NotImplementedError("frhip.optim.SGD: dampening / nesterov / maximize are not implemented")
        idx, rows = p._frhip_row_grad
        if not (p.is_cuda and p.is_contiguous() and p.dtype == torch.float32 and p.dim() in (1, 2)):
            raise _lib.FrhipError("frhip.optim.SGD: a row gradient needs a contiguous float32 [n, D] or [n] ROCm parameter")
        D = p.shape[1] if p.dim() == 2 else 1
        if (idx.dtype != torch.int32 or idx.dim() != 1 or idx.shape[0] > p.shape[0] or rows.dtype != torch.float32
                or tuple(rows.shape) != (idx.shape[0],) + tuple(p.shape[1:])):
            raise _lib.FrhipError("frhip.optim.SGD: row gradient of shape %s with %s indices of %s for a parameter of shape %s"
                                  % (tuple(rows.shape), tuple(idx.shape), idx.dtype, tuple(p.shape)))
        state = self.state[p]
        buf = state.get("momentum_buffer")
        if buf is None:  # first use; torch.optim.SGD writes None before its first step
            buf = state["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        if buf.shape != p.shape or not buf.is_contiguous():
            raise _lib.FrhipError("frhip.optim.SGD: param / momentum buffer must share one dense layout")
        if ctl is None:
            ops.call("fr_sgd_rows", p, buf, rows.contiguous(), idx.contiguous(), idx.shape[0], D, float(group["lr"]),
                     float(group["momentum"]), float(group["weight_decay"]), st)()
        else:  # under a GradGuard: the go flag only, the head is not clipped
            ops.call("fr_sgd_rows_ctl", p, buf, rows.contiguous(), idx.contiguous(), idx.shape[0], D, float(group["lr"]),
                     float(group["momentum"]), float(group["weight_decay"]), ctl, st)()
        p._frhip_row_grad = None


class Adam(torch.optim.Optimizer):
    """``torch.optim.Adam(params, lr)`` with its defaults (betas (0.9, 0.999), eps 1e-8, no weight decay, no amsgrad) as one
    multi-tensor HIP launch per parameter group -- the reference's ``OPTIMIZER_NAME == 'Adam'`` branch (train.py:197-198).
    State keys and layout follow torch (``step`` as a host float tensor, ``exp_avg``, ``exp_avg_sq``), so state dicts
    are interchangeable with ``torch.optim.Adam``.  Parameters whose ``.grad`` is None are skipped and keep their step.

    ``step(guard=...)`` as ``SGD.step``.  On a step the guard skips, ``exp_avg``, ``exp_avg_sq`` and the parameters keep their
    bits, but the host ``step`` counter still advances -- the host does not know that the device skipped -- so the bias
    correction of later steps is one step ahead of a run that never skipped."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))
        self._sig = None
        self._tables = []  # [group index, step value before this update, table_dev, chunks_dev, nchunks, params, use_coef]

    zero_grad = SGD.zero_grad

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._sig = None

    def _relaid(self, p, t):
        if t.shape == p.shape and not _dense_same(p, t):
            r = torch.empty_like(p, memory_format=torch.preserve_format)
            r.copy_(t)
            return r
        return t

    def _build(self, guard=None):
        for group in self.param_groups:  # a loaded state dict may carry settings this kernel does not implement
            if group.get("dampening", 0) != 0 or group.get("nesterov", False) or group.get("maximize", False):
                raise NotImplementedError("frhip.optim.Adam: dampening / nesterov / maximize are not implemented")
        chunk = _lib.lib.fr_sgd_chunk_elems()
        self._tables = []
        for gi, group in enumerate(self.param_groups):
            by_step = {}
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not p.is_cuda:
                    raise _lib.FrhipError("frhip.optim.Adam: parameter on %s -- the HIP optimizer needs ROCm tensors"
                                          % p.device)
                st = self.state[p]
                if "step" not in st:
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg"], st["exp_avg_sq"] = self._relaid(p, st["exp_avg"]), self._relaid(p, st["exp_avg_sq"])
                if not (_dense_same(p, p.grad) and _dense_same(p, st["exp_avg"]) and _dense_same(p, st["exp_avg_sq"])):
                    raise _lib.FrhipError("frhip.optim.Adam: param / grad / moments must share one dense layout")
                # with a guard: its parameter set (clipped) apart from the rest (go flag only)
                by_step.setdefault((float(st["step"]), 1 if guard is not None and guard.covers(p) else 0), []).append(p)
            for (step0, use_coef), plist in by_step.items():
                arr = (_lib.FrAdamTensor * len(plist))()
                chunks = []
                for i, p in enumerate(plist):
                    st = self.state[p]
                    arr[i].p, arr[i].g = p.data_ptr(), p.grad.data_ptr()
                    arr[i].m, arr[i].v, arr[i].n = st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel()
                    chunks.extend((i, c) for c in range((p.numel() + chunk - 1) // chunk))
                dev = plist[0].device
                raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
                ch = torch.tensor(chunks, dtype=torch.int32).reshape(-1).to(dev)
                self._tables.append([gi, step0, raw, ch, len(chunks), plist, use_coef])

    def _signature(self):
        return tuple((p.data_ptr(), 0 if p.grad is None else p.grad.data_ptr())
                     for g in self.param_groups for p in g["params"])

    @torch.no_grad()
    def step(self, closure=None, guard=None):
        loss = closure() if closure is not None else None
        ctl = guard._take("frhip.optim.Adam") if guard is not None else None
        for _group, _p in _row_grad_params(self.param_groups):
            raise NotImplementedError("frhip.optim.Adam: a parameter carries a row gradient (ShardedMarginLoss with "
                                      "sparse_update=True); the row-sparse update is built for frhip.optim.SGD only -- run "
                                      "Adam with sparse_update=False")
        sig = (self._signature(), None if guard is None else guard.key)
        if sig != self._sig:
            if guard is None:
                self._build()
            else:
                self._build(guard)
            self._sig = sig
        st = ops.current_stream_ptr()
        for rec in self._tables:
            gi, step0, raw, ch, n, plist, use_coef = rec
            group = self.param_groups[gi]
            b1, b2 = group["betas"]
            step = step0 + 1.0
            # the scalars torch computes in double on the host (torch/optim/adam.py, _single_tensor_adam)
            step_size = group["lr"] / (1.0 - b1 ** step)
            bc2_sqrt = (1.0 - b2 ** step) ** 0.5
            table = ctypes.cast(ctypes.c_void_p(raw.data_ptr()), ctypes.POINTER(_lib.FrAdamTensor))
            scalars = [float(step_size), float(1.0 - b1), float(b2), float(1.0 - b2), float(group["eps"]), float(bc2_sqrt)]
            if ctl is None:
                ops.Launch("fr_adam_step", [table, ctypes.c_void_p(ch.data_ptr()), n] + scalars + [st])()
            else:
                ops.Launch("fr_adam_step_ctl", [table, ctypes.c_void_p(ch.data_ptr()), n] + scalars +
                           [ops.ptr(ctl), use_coef, st])()
            for p in plist:
                self.state[p]["step"] += 1.0
            rec[1] = step
        return loss


class ParamEMA(object):
    """``dst = alpha * dst + (1 - alpha) * src`` over the parameters of two modules of the same class, as ONE multi-tensor HIP
    launch per ``step()``: the gallery network of semi-siamese training (``head.metrics.SST_Prototype``) following the probe
    network.  Buffers are not touched: a gallery network keeps its own BatchNorm statistics.  The kernel takes ``a =
    float(alpha)`` and ``b = float(1.0 - alpha)`` (the subtraction in double) and rounds the two products and the sum to fp32
    one by one; on host parameters ``step()`` runs the same expression in torch.  The launch table is cached on the
    tensors' addresses, as ``SGD``'s."""

    def __init__(self, dst_module, src_module, alpha=0.999):
        dst, src = list(dst_module.named_parameters()), list(src_module.named_parameters())
        if [n for n, _ in dst] != [n for n, _ in src]:
            raise ValueError("frhip.optim.ParamEMA: the two modules must have the same parameters, in the same order")
        self.pairs = [(d, s) for (_, d), (_, s) in zip(dst, src)]
        self.alpha = float(alpha)
        self._sig = None
        self._table = None  # (table_dev, chunks_dev, nchunks)

    def _signature(self):
        return tuple((d.data_ptr(), s.data_ptr()) for d, s in self.pairs)

    def _build(self):
        chunk = _lib.lib.fr_ema_chunk_elems()
        arr = (_lib.FrEmaTensor * len(self.pairs))()
        chunks = []
        for i, (d, s) in enumerate(self.pairs):
            if d.device != s.device or d.dtype != torch.float32 or s.dtype != torch.float32:
                raise _lib.FrhipError("frhip.optim.ParamEMA: both parameters must be float32 tensors on one device")
            if not _dense_same(d, s):
                raise _lib.FrhipError("frhip.optim.ParamEMA: the two parameters must share one dense layout")
            arr[i].dst, arr[i].src, arr[i].n = d.data_ptr(), s.data_ptr(), d.numel()
            chunks.extend((i, c) for c in range((d.numel() + chunk - 1) // chunk))
        dev = self.pairs[0][0].device
        raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
        ch = torch.tensor(chunks, dtype=torch.int32).reshape(-1).to(dev)
        self._table = (raw, ch, len(chunks))

    @torch.no_grad()
    def step(self):
        if not self.pairs:
            return
        a, b = self.alpha, 1.0 - self.alpha
        devices = set(t.device.type for pair in self.pairs for t in pair)
        if devices == {"cpu"}:
            for d, s in self.pairs:
                if not _dense_same(d, s):
                    raise _lib.FrhipError("frhip.optim.ParamEMA: the two parameters must share one dense layout")
                d.copy_(d * a + s * b)  # two products and a sum, each rounded on its own: what the kernel computes
            return
        if devices != {"cuda"}:
            raise _lib.FrhipError("frhip.optim.ParamEMA: the parameters of both modules must live on one device")
        sig = self._signature()
        if sig != self._sig:
            self._build()
            self._sig = sig
        raw, ch, n = self._table
        table = ctypes.cast(ctypes.c_void_p(raw.data_ptr()), ctypes.POINTER(_lib.FrEmaTensor))  # device array
        ops.Launch("fr_ema_step", [table, ctypes.c_void_p(ch.data_ptr()), n, float(a), float(b),
                                   ops.current_stream_ptr()])()


_GUARD_KEYS = itertools.count(1)


class GradGuard(object):
    """Global-norm gradient clipping and the non-finite step skip, decided on the device.

        guard = GradGuard(backbone.parameters(), max_norm=5.0, skip_nonfinite=True)
        loss.backward(); guard.measure(); optimizer.step(guard=guard)

    ``measure()`` enqueues two launches on the current stream: fr_grad_sumsq (one workgroup per 4096-element chunk of every
    dense ``.grad`` of ``params``, the sum of squares in double in a fixed order) and fr_grad_guard (one workgroup), which
    leaves in ``self.ctl`` (device float32 [4]) the L2 norm, the clip coefficient of ``torch.nn.utils.clip_grad_norm_``
    (``min(1, max_norm / (norm + 1e-6))`` in fp32; 1 when ``max_norm`` is None: measure only), the go flag (0 when
    ``skip_nonfinite`` and the sum of squares is inf or NaN) and a zero, and counts in ``self.skipped`` (device int32 [2])
    the skipped steps and all measured steps.  No host read, no synchronisation, no allocation after the first call; the
    result is bit-identical from run to run.  ``optimizer.step(guard=guard)`` then runs under that control word; calling it
    without a ``measure()`` since the last step raises.  ``state_dict()`` is the one place that reads the device.

    Norm type 2 only.  Parameters whose ``.grad`` is None are left out (a frozen body; a parameter that carries a row
    gradient), and the table is rebuilt when the gradients' addresses change.  ``.grad`` is never written: the optimizer
    applies the coefficient as it reads the gradient (torch scales in place).

    The norm is meant for the backbone alone, as in the Partial-FC recipe -- and under a class-sharded head it must be:
    every rank holds another shard, so a norm that included it would differ between the ranks and the replicated backbone
    would diverge.  After ``DataParallel.synchronize()`` the backbone's gradients are the same bits on every rank, hence so
    are the coefficient and the skip decision, without a collective.  Parameters outside the set (the head) are not
    clipped but obey the go flag.

    Not protected: buffers that move in the forward pass move on a skipped step too -- BatchNorm running statistics,
    CurricularFace's ``t``, AdaCos's scale, SphereFace's ``iter`` -- as under ``torch.cuda.amp.GradScaler``."""

    def __init__(self, params, max_norm=None, skip_nonfinite=True, norm_type=2.0):
        self.params = list(params)
        if not self.params:
            raise ValueError("frhip.optim.GradGuard: no parameters")
        if float(norm_type) != 2.0:
            raise NotImplementedError("frhip.optim.GradGuard: norm type 2 only, got %r" % (norm_type,))
        if max_norm is not None:
            if isinstance(max_norm, bool) or not isinstance(max_norm, (int, float)) or not max_norm > 0:
                raise ValueError("frhip.optim.GradGuard: max_norm must be a number greater than 0, or None to measure "
                                 "without clipping; got %r" % (max_norm,))
        for p in self.params:
            if not p.is_cuda:
                raise _lib.FrhipError("frhip.optim.GradGuard: parameter on %s -- the HIP guard needs ROCm tensors" % p.device)
        self.max_norm = None if max_norm is None else float(max_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        dev = self.params[0].device
        self.ctl = torch.zeros(4, dtype=torch.float32, device=dev)
        self.skipped = torch.zeros(2, dtype=torch.int32, device=dev)
        self._ids = frozenset(id(p) for p in self.params)
        self.key = next(_GUARD_KEYS)  # the optimizers key their launch tables on it: the parameter set never changes
        self._sig = None
        self._table = None  # (table_dev, chunks_dev, nchunks, parts)
        self._measured = False

    def covers(self, p):
        return id(p) in self._ids

    def _signature(self):
        return tuple(0 if p.grad is None else p.grad.data_ptr() for p in self.params)

    def _build(self):
        chunk = _lib.lib.fr_sgd_chunk_elems()
        recs, chunks = [], []
        for p in self.params:
            g = p.grad
            if g is None:
                continue
            if not g.is_cuda or g.dtype != torch.float32 or g.is_sparse or not _is_dense(g):
                raise _lib.FrhipError("frhip.optim.GradGuard: a gradient must be a dense float32 ROCm tensor")
            t = len(recs)
            recs.append((g.data_ptr(), g.numel()))
            chunks.extend((t, c) for c in range((g.numel() + chunk - 1) // chunk))
        dev = self.ctl.device
        if not chunks:
            self._table = (None, None, 0, None)
            return
        arr = (_lib.FrGradTensor * len(recs))()
        for i, (gp, n) in enumerate(recs):
            arr[i].g, arr[i].n = gp, n
        raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
        ch = torch.tensor(chunks, dtype=torch.int32).reshape(-1).to(dev)
        self._table = (raw, ch, len(chunks), torch.zeros(len(chunks), dtype=torch.float64, device=dev))

    @torch.no_grad()
    def measure(self):
        """Enqueue the norm and the control word of the gradients as they are now; returns ``self.ctl`` (device)."""
        sig = self._signature()
        if sig != self._sig:
            self._build()
            self._sig = sig
        raw, ch, n, parts = self._table
        st = ops.current_stream_ptr()
        if n:
            table = ctypes.cast(ctypes.c_void_p(raw.data_ptr()), ctypes.POINTER(_lib.FrGradTensor))  # device array
            ops.Launch("fr_grad_sumsq", [table, ctypes.c_void_p(ch.data_ptr()), n, ops.ptr(parts), st])()
        ops.Launch("fr_grad_guard", [ops.ptr(parts), n, 0.0 if self.max_norm is None else self.max_norm,
                                     int(self.skip_nonfinite), ops.ptr(self.ctl), ops.ptr(self.skipped), st])()
        self._measured = True
        return self.ctl

    def _take(self, who):
        """The control word for one optimizer step; a host flag, no device read."""
        if not self._measured:
            raise _lib.FrhipError("%s: step(guard=...) without a GradGuard.measure() for this step -- call guard.measure() "
                                  "after backward (and after the gradient all-reduce) and before step" % who)
        self._measured = False
        return self.ctl

    def state_dict(self):
        """{"skipped": steps the guard skipped, "steps": steps it measured}.  Reads the device (a synchronisation): for
        checkpoints and display lines."""
        skipped, steps = (int(v) for v in self.skipped.tolist())
        return {"skipped": skipped, "steps": steps}

    def load_state_dict(self, state):
        self.skipped.copy_(torch.tensor([int(state["skipped"]), int(state["steps"])], dtype=torch.int32))


def _row_grad_params(param_groups):
    """[(group, parameter)] of the parameters that carry a pending ``_frhip_row_grad`` (frhip/sharded_head.py)."""
    return [(g, p) for g in param_groups for p in g["params"] if getattr(p, "_frhip_row_grad", None) is not None]


def _dense_same(a, b):
    return a.shape == b.shape and a.stride() == b.stride() and _is_dense(a)


def _is_dense(t):
    """True when the tensor's elements occupy one contiguous run of memory (any permutation of a dense layout)."""
    if t.numel() == 0:
        return True
    dims = sorted((s, n) for s, n in zip(t.stride(), t.shape) if n > 1)
    expect = 1
    for s, n in dims:
        if s != expect:
            return False
        expect *= n
    return True
