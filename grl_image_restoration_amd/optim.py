"""Multi-tensor AdamW for the training path (BASELINE config 5).

The reference trains GRL with ``torch.optim.AdamW`` (config/optimizer/adamw.yaml: lr 2e-4, weight_decay 1e-4, torch defaults
otherwise; built in engines/base.py:451-470) over 1390 parameter tensors; a per-tensor update is host-launch bound.  ``FusedAdamW`` performs the
identical update (decoupled weight decay, bias correction as in torch.optim.AdamW, no amsgrad) for ALL tensors of a
parameter group in ONE launch of ``grl_adamw_step`` (csrc/grad.hip): a host-built list of 4096-element chunks, pointer tables
in device memory.  fp32 parameters on the GPU; CPU parameters take the same update as plain torch arithmetic (``_step_cpu``: like the
model's composite path it exists so that a module built without a GPU steps instead of raising -- never reached by GPU tensors).

Two stabilisers ride in the same launches (ABI 44), so that neither costs a pass of its own over the 77 MB of GRL-Base:
  * ``max_grad_norm``: clipping by the GLOBAL norm over all groups, as ``torch.nn.utils.clip_grad_norm_`` over all parameters
    (Restormer's ``use_grad_clip``).  ``grl_grad_sqnorm`` reads the gradients once (per-chunk sums of squares in double, no atomics:
    bit-reproducible), ``grl_grad_clip_finish`` turns them into {coefficient, norm} in device memory, and the AdamW launch multiplies
    its gradient scale by the coefficient: the gradients are never rewritten and the host reads nothing, so the step stays capturable.
  * ``ema_decay``: an exponential moving average of the weights (BasicSR's ``params_ema``: e <- e + (1 - decay) (w' - e), started as
    a copy of the weights before the first step), updated by the AdamW launch from the new weight while it is in a register.
    ``state[p]["ema"]`` travels in ``state_dict()``; ``ema_state_dict`` / ``ema_applied`` hand the averaged model out.
"""
import contextlib
from typing import Iterable

import torch

from . import _lib as L

_CHUNK = 4096


class FusedAdamW(torch.optim.Optimizer):
    def __init__(self, params: Iterable, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None,
                 ema_decay=None):
        if lr < 0 or eps < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1) or weight_decay < 0:
            raise ValueError("invalid AdamW hyper-parameter")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm,
                                      ema_decay=ema_decay))
        self._max_grad_norm()         # (validates the groups: one positive norm for all of them, 0 <= ema_decay < 1)
        self._tables = {}
        self._clip = None         # clipping: the partial sums (double) and {coefficient, norm} (fp32) in device memory
        self._clip_last = None    # where the last step left {coefficient, norm}: the device buffer, or host floats (CPU path)
        self._step_dev = None     # capture mode (enable_capture): per group, the step count as a device tensor
        self._hyper_dev = {}      # capture mode: per group, {lr, weight_decay} as a device tensor the captured launch reads
        self._frozen = {}         # capture mode: per group, the hyper-parameters a captured launch holds BY VALUE (betas, eps)
        self._pinned = {}         # per group: pinned host table of gradient pointers of the NEXT capture (one table per capture:
        self._pinned_all = []     # a replay copies from the table of its own graph; all of them are kept alive here)

    def _group_tables(self, gi, plist):
        """Device pointer / size tables of a parameter group (rebuilt when the set of tensors or their storage changes)."""
        # (the moment buffers are part of the key: load_state_dict replaces them while the parameters stay where they are)
        ema_ptr = lambda p: self.state[p]["ema"].data_ptr() if "ema" in self.state[p] else 0
        key = tuple((p.data_ptr(), p.numel(), self.state[p]["exp_avg"].data_ptr(), self.state[p]["exp_avg_sq"].data_ptr(), ema_ptr(p))
                    for p in plist)
        ent = self._tables.get(gi)
        if ent is not None and ent["key"] == key:
            return ent
        dev = plist[0].device
        i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)
        chunk_t, chunk_o = [], []
        for t, p in enumerate(plist):
            for off in range(0, p.numel(), _CHUNK):
                chunk_t.append(t)
                chunk_o.append(off)
        st = [self.state[p] for p in plist]
        ent = dict(
            key=key,
            params=i64([p.data_ptr() for p in plist]),
            exp_avg=i64([s["exp_avg"].data_ptr() for s in st]),
            exp_avg_sq=i64([s["exp_avg_sq"].data_ptr() for s in st]),
            ema=i64([s["ema"].data_ptr() for s in st]) if all("ema" in s for s in st) else None,
            numel=i64([p.numel() for p in plist]),
            chunk_tensor=torch.tensor(chunk_t, dtype=torch.int32, device=dev),
            chunk_offset=i64(chunk_o),
            n=len(chunk_t),
        )
        self._tables[gi] = ent
        return ent

    def _max_grad_norm(self):
        """The clipping norm of ALL groups (None: off).  The norm is global, as ``clip_grad_norm_`` over all parameters is, so
        the groups must agree; the per-group ``ema_decay`` is validated along the way."""
        norms = {g.get("max_grad_norm") for g in self.param_groups}
        if len(norms) > 1:
            raise ValueError(f"FusedAdamW: max_grad_norm must be the same in all parameter groups (the norm is global), got {sorted(map(str, norms))}")
        mn = norms.pop() if norms else None
        if mn is not None and not mn > 0:
            raise ValueError(f"FusedAdamW: max_grad_norm must be positive, got {mn}")
        for g in self.param_groups:
            d = g.get("ema_decay")
            if d is not None and not 0 <= d < 1:
                raise ValueError(f"FusedAdamW: ema_decay must be in [0, 1), got {d}")
        return mn

    def _clip_buffers(self, layout, dev):
        """Partial sums (one double per chunk, the groups one after the other) and the two-float output of the clipped step.
        Allocated with the group tables -- on the first eager step, or when the chunk layout changes -- never during a capture:
        a captured launch holds their addresses."""
        ent = self._clip
        if ent is not None and ent["key"] == (dev, layout):
            return ent
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("FusedAdamW: the set of clipped gradients changed; run an eager step before capturing")
        base, total = {}, 0
        for gi, n in layout:
            base[gi] = total
            total += n
        out = ent["out"] if ent is not None and ent["key"][0] == dev else torch.zeros(2, dtype=torch.float32, device=dev)
        self._clip = dict(key=(dev, layout), base=base, total=total, out=out,
                          partials=torch.zeros(total, dtype=torch.float64, device=dev))
        return self._clip

    def last_grad_norm(self) -> float:
        """The global gradient norm the last clipped step measured (of the scaled gradient: the averaged one in a data-parallel
        step).  A host read: for logging and tests, not for the step."""
        return self._clip_read()[1]

    def last_clip_coef(self) -> float:
        """The coefficient the last clipped step multiplied its gradients by: min(1, max_grad_norm / (norm + 1e-6))."""
        return self._clip_read()[0]

    def _clip_read(self):
        if self._clip_last is None:
            raise RuntimeError("FusedAdamW: no clipped step has run (max_grad_norm is None, or step() was not called yet)")
        if torch.is_tensor(self._clip_last):
            coef, norm = self._clip_last.cpu().tolist()
            return coef, norm
        return self._clip_last

    def ema_state_dict(self, model: torch.nn.Module) -> dict:
        """``model.state_dict()`` with every optimized parameter replaced by (a copy of) its average; buffers, and parameters
        without an average, are as they are."""
        sd = model.state_dict()
        for name, p in model.named_parameters():
            s = self.state.get(p)
            if s is not None and "ema" in s and name in sd:
                sd[name] = s["ema"].detach().clone().view_as(p)
        return sd

    @contextlib.contextmanager
    def ema_applied(self, model: torch.nn.Module):
        """Inside the context the model's optimized parameters hold their averages (validation of the averaged model); afterwards
        the trained weights are back.  Contents are copied, no pointer is swapped -- a captured graph and the pointer tables hold
        the parameters' addresses -- and the copies bump the parameters' versions, so the inference plan sees both changes."""
        pairs = [(p, self.state[p]["ema"]) for p in model.parameters() if p in self.state and "ema" in self.state[p]]
        saved = [p.detach().clone() for p, _ in pairs]
        with torch.no_grad():
            for p, e in pairs:
                p.copy_(e.view_as(p))
        try:
            yield model
        finally:
            with torch.no_grad():
                for (p, _), w in zip(pairs, saved):
                    p.copy_(w)

    def load_state_dict(self, state_dict):
        """Accepts this class's own state and the one of ``torch.optim.AdamW`` (what the reference's Lightning checkpoints hold
        under ``optimizer_states``: ``step`` as a 0-dim tensor per parameter)."""
        # capture mode: a captured launch holds the ADDRESSES of the moment buffers, of the pointer tables and of the step counters.
        # The loaded values therefore go INTO the existing buffers (torch's load_state_dict would replace the tensors: a replay
        # would keep updating the old moments and ignore the loaded ones -- ADVICE r4), and the tables stay.
        keep = {}
        if self._step_dev:
            keep = {p: {k: s[k] for k in self._BUFFERS if k in s} for p, s in self.state.items() if "exp_avg" in s}
        # (a state saved by torch.optim.AdamW, or before ABI 44, has no max_grad_norm / ema_decay in its groups: the constructor's stay)
        own = [(g.get("max_grad_norm"), g.get("ema_decay")) for g in self.param_groups]
        super().load_state_dict(state_dict)
        for g, (mn, d) in zip(self.param_groups, own):
            g.setdefault("max_grad_norm", mn)
            g.setdefault("ema_decay", d)
        self._max_grad_norm()
        self._normalise_state()
        if keep:
            with torch.no_grad():
                for p, old in keep.items():
                    s = self.state.get(p)
                    if s is None or "exp_avg" not in s:
                        continue
                    for k, buf in old.items():
                        if k not in s:            # (only `ema` can be missing: the average starts again from the current weights)
                            buf.copy_(p); s[k] = buf
                        elif s[k] is not buf:
                            buf.copy_(s[k]); s[k] = buf
            for gi, group in enumerate(self.param_groups):
                steps = {int(self.state[p]["step"]) for p in group["params"] if p in self.state and "step" in self.state[p]}
                if len(steps) == 1:
                    self._step_dev[gi].fill_(steps.pop())
            self.refresh_capture_hyper()
        else:
            self._tables = {}

    _BUFFERS = ("exp_avg", "exp_avg_sq", "ema")      # per-parameter state a launch addresses through the pointer tables

    def state_dict(self):
        """(In capture mode the step counts live on the device: they are read back first.)"""
        self.sync_step_from_device()
        return super().state_dict()

    def __setstate__(self, state):
        super().__setstate__(state)
        # (groups without max_grad_norm / ema_decay -- torch.optim.AdamW's, or older ones -- are read with .get; load_state_dict,
        # which comes through here, fills them from the constructor's afterwards)
        self.__dict__.setdefault("_clip", None)
        self.__dict__.setdefault("_clip_last", None)
        if not getattr(self, "_step_dev", None):   # (capture mode: load_state_dict keeps buffers and tables, see there)
            self._tables = {}
        self._normalise_state()

    def _normalise_state(self):
        for p, s in self.state.items():
            if "step" in s and torch.is_tensor(s["step"]):
                s["step"] = int(s["step"].item())
            for k in self._BUFFERS:
                if k in s and (s[k].dtype != torch.float32 or not s[k].is_contiguous() or s[k].device != p.device):
                    s[k] = s[k].to(device=p.device, dtype=torch.float32).contiguous()

    def enable_capture(self):
        """Makes ``step()`` replayable from a HIP graph (train_graph.GraphedTrainStep): the step count moves to device memory
        (incremented by a captured op; the bias corrections are computed from it on the device, in float64 like the host path,
        and handed to the kernel as GrlAdamWArgs.bias_corrections_dev) and the table of gradient pointers is copied from pinned
        host memory.  Call after at least one eager step (the moments must exist)."""
        first = not self._step_dev
        if not first:                            # already in capture mode (a second graph): the device counters are the truth and
            self.sync_step_from_device()         # keep their addresses -- an earlier graph increments them too
        else:
            self._step_dev = {}
        for gi, group in enumerate(self.param_groups):
            dev = group["params"][0].device
            if first:
                steps = {int(self.state[p]["step"]) for p in group["params"] if p in self.state and "step" in self.state[p]}
                if len(steps) != 1:
                    raise RuntimeError("FusedAdamW.enable_capture: run an eager step first (every parameter of a group needs the same step count)")
                self._step_dev[gi] = torch.full((1,), steps.pop(), dtype=torch.int64, device=dev)
                self._hyper_dev[gi] = torch.tensor([group["lr"], group["weight_decay"]], dtype=torch.float32, device=dev)
                self._frozen[gi] = self._held_by_value(group)
            # ONE pinned table of gradient pointers PER CAPTURE (allocated here: pinning host memory is not allowed while a stream is
            # capturing).  A shared table would be overwritten by the next capture, and a replay of the earlier graph would then
            # update from another graph's gradient buffers.
            host = torch.zeros(len(group["params"]), dtype=torch.int64)
            host = host.pin_memory() if dev.type == "cuda" else host
            self._pinned[gi] = host
            self._pinned_all.append(host)

    @staticmethod
    def _held_by_value(group):
        return (tuple(group["betas"]), group["eps"], group.get("max_grad_norm"), group.get("ema_decay"))

    def refresh_capture_hyper(self):
        """Capture mode: brings the device copy of {lr, weight_decay} up to date with ``param_groups`` -- call before every replay
        of a captured step (GraphedTrainStep does), so that LR schedulers act on replays.  betas / eps / max_grad_norm /
        ema_decay are held by value in a captured launch: changing them after a capture raises here instead of being silently
        ignored."""
        if not self._step_dev:
            return
        for gi, group in enumerate(self.param_groups):
            if self._frozen.get(gi) != self._held_by_value(group):
                raise RuntimeError("FusedAdamW: betas / eps / max_grad_norm / ema_decay changed after a step was captured; they are "
                                   "frozen in the graph -- re-capture")
            hd = self._hyper_dev[gi]
            want = (float(group["lr"]), float(group["weight_decay"]))
            if getattr(hd, "_host_copy", None) != want:
                hd.copy_(torch.tensor(want, dtype=torch.float32))
                hd._host_copy = want

    def sync_step_from_device(self):
        """After graph replays: the host-side ``state[p]['step']`` (what state_dict() saves) <- the device counters."""
        if self._step_dev:
            for gi, group in enumerate(self.param_groups):
                n = int(self._step_dev[gi].item())
                for p in group["params"]:
                    if p in self.state and "step" in self.state[p]:
                        self.state[p]["step"] = n

    def _clip_cpu(self, work, grad_scale, max_norm):
        """{coefficient, norm} of the CPU path, by the expressions of grl_grad_clip_finish: the sum of squares in float64, norm and
        coefficient in float64 (torch.clamp's treatment of inf / NaN), each rounded once to fp32."""
        total = torch.zeros((), dtype=torch.float64)
        for _, _, plist in work:
            for p in plist:
                total += p.grad.detach().double().square().sum()
        norm = total.sqrt() * abs(float(grad_scale))
        coef = (max_norm / (norm + 1e-6)).clamp(max=1.0)
        self._clip_last = (coef.float().item(), norm.float().item())
        return coef.float()

    def _step_cpu(self, group, plist, grad_scale, clip_coef=None):
        """torch.optim.AdamW's single-tensor update on CPU tensors (decoupled weight decay, bias correction), gradients multiplied by
        ``grad_scale`` (times the clip coefficient, the product formed in fp32 as the kernel forms it) first, and the weight average
        moved by ``torch.lerp`` afterwards.  Exists for the same reason as the model's composite path (composite.py): a module built without a GPU
        -- the gloo tests of the data-parallel step, a unit test of a surrounding engine -- steps instead of raising.  Never reached
        by GPU parameters; nothing here is timed or claimed as MI355X work."""
        b1, b2 = group["betas"]
        lr, wd, eps = group["lr"], group["weight_decay"], group["eps"]
        decay = group.get("ema_decay")
        if clip_coef is not None:
            grad_scale = (torch.tensor(grad_scale, dtype=torch.float32) * clip_coef).item()
        for p in plist:
            s = self.state[p]
            if not s:
                s["step"] = 0
                s["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                s["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            if decay is not None and "ema" not in s:     # BasicSR's initialisation: a copy of the weights before the update
                s["ema"] = p.detach().clone(memory_format=torch.contiguous_format)
            s["step"] = int(s["step"]) + 1
            g = p.grad * grad_scale if grad_scale != 1.0 else p.grad
            p.mul_(1.0 - lr * wd)
            s["exp_avg"].lerp_(g, 1.0 - b1)
            s["exp_avg_sq"].mul_(b2).addcmul_(g, g, value=1.0 - b2)
            bc1, bc2s = 1.0 - b1 ** s["step"], (1.0 - b2 ** s["step"]) ** 0.5
            p.addcdiv_(s["exp_avg"], (s["exp_avg_sq"].sqrt() / bc2s).add_(eps), value=-lr / bc1)
            if decay is not None:
                s["ema"].lerp_(p.detach(), 1.0 - decay)
        torch.autograd.graph.increment_version(plist)

    @torch.no_grad()
    def step(self, closure=None, grad_scale: float = 1.0):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        L.lib()    # a missing or stale library is an error even when every group is on the CPU
        work = [(gi, group, [p for p in group["params"] if p.grad is not None]) for gi, group in enumerate(self.param_groups)]
        work = [w for w in work if w[2]]
        max_norm = self._max_grad_norm()
        on_cpu = [all(not p.is_cuda for p in plist) for _, _, plist in work]
        if max_norm is not None and work and (len({plist[0].device for _, _, plist in work}) != 1 or (any(on_cpu) and not all(on_cpu))):
            raise RuntimeError("FusedAdamW: max_grad_norm needs all parameter groups on one device (the norm is global)")
        clip_cpu = self._clip_cpu(work, grad_scale, max_norm) if (max_norm is not None and work and all(on_cpu)) else None
        launches = []
        for (gi, group, plist), cpu in zip(work, on_cpu):
            if cpu:                                     # CPU tensors: the same update as plain torch arithmetic (module docstring)
                self._step_cpu(group, plist, grad_scale, clip_cpu)
                continue
            decay = group.get("ema_decay")
            for p in plist:
                if (not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous() or p.grad.dtype != torch.float32
                        or not p.grad.is_contiguous()):
                    raise RuntimeError("FusedAdamW: fp32 contiguous GPU parameters only (a group is either all on the GPU or all on the CPU)")
                s = self.state[p]
                if not s:
                    s["step"] = 0
                    s["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    s["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                if decay is not None and "ema" not in s:     # BasicSR's initialisation: a copy of the weights before the update
                    if torch.cuda.is_current_stream_capturing():
                        raise RuntimeError("FusedAdamW: run an eager step before capturing (the weight averages must exist)")
                    s["ema"] = p.detach().clone(memory_format=torch.contiguous_format)
            steps = {int(self.state[p]["step"]) for p in plist}
            if len(steps) != 1:
                raise RuntimeError("FusedAdamW: parameters of one group must share their step count")
            step = steps.pop() + 1
            capturing = torch.cuda.is_current_stream_capturing()
            if capturing and self._step_dev is None:
                raise RuntimeError("FusedAdamW: call enable_capture() before capturing step() in a graph")
            if not capturing:              # (a captured step does not execute: the device counter advances on replay only)
                for p in plist:
                    self.state[p]["step"] = step
            b1, b2 = group["betas"]
            bc_dev = None
            if self._step_dev is not None and not capturing:
                self.refresh_capture_hyper()      # (eager steps between replays read the same device copy)
            if self._step_dev is not None:
                sd = self._step_dev[gi]
                sd.add_(1)
                t = sd.double()
                bc_dev = torch.cat([1.0 - b1 ** t, (1.0 - b2 ** t).sqrt()]).float()   # (1 - 0.999^t cancels in float32: 6e-5 off at t = 2)
            ent = self._group_tables(gi, plist)
            if capturing:
                host = self._pinned[gi][: len(plist)]
                host.copy_(torch.tensor([p.grad.data_ptr() for p in plist], dtype=torch.int64))
                grads = host.to(plist[0].device, non_blocking=True)
            else:
                grads = torch.tensor([p.grad.data_ptr() for p in plist], dtype=torch.int64, device=plist[0].device)
            launches.append((gi, group, plist, ent, grads, step, bc_dev))
        clip = None
        if max_norm is not None and launches:
            # the global norm first: every group's sums of squares into one buffer, one finishing launch, and the AdamW launches
            # below read its coefficient from device memory.  grad_scale goes into the norm: it is that of the scaled gradient.
            clip = self._clip_buffers(tuple((gi, ent["n"]) for gi, _, _, ent, _, _, _ in launches), launches[0][2][0].device)
            for gi, _, _, ent, grads, _, _ in launches:
                L.launch("grl_grad_sqnorm", L.GrlGradNormArgs(
                    grads=grads.data_ptr(), numel=ent["numel"].data_ptr(), chunk_tensor=ent["chunk_tensor"].data_ptr(),
                    chunk_offset=ent["chunk_offset"].data_ptr(), num_chunks=ent["n"], partials=clip["partials"].data_ptr(),
                    base=clip["base"][gi]))
            L.launch("grl_grad_clip_finish", L.GrlGradClipArgs(
                partials=clip["partials"].data_ptr(), n_partials=clip["total"], grad_scale=grad_scale, max_norm=max_norm,
                out=clip["out"].data_ptr()))
            self._clip_last = clip["out"]
        for gi, group, plist, ent, grads, step, bc_dev in launches:
            b1, b2 = group["betas"]
            decay = group.get("ema_decay")
            args = L.GrlAdamWArgs(
                params=ent["params"].data_ptr(), grads=grads.data_ptr(), exp_avg=ent["exp_avg"].data_ptr(),
                exp_avg_sq=ent["exp_avg_sq"].data_ptr(), numel=ent["numel"].data_ptr(), weight_decay_flags=None,
                chunk_tensor=ent["chunk_tensor"].data_ptr(), chunk_offset=ent["chunk_offset"].data_ptr(), num_chunks=ent["n"],
                lr=group["lr"], beta1=b1, beta2=b2, eps=group["eps"], weight_decay=group["weight_decay"],
                bias_correction1=1.0 - b1 ** step, bias_correction2_sqrt=(1.0 - b2 ** step) ** 0.5, grad_scale=grad_scale,
                bias_corrections_dev=bc_dev.data_ptr() if bc_dev is not None else None,
                hyper_dev=self._hyper_dev[gi].data_ptr() if (self._step_dev is not None and gi in self._hyper_dev) else None,
                grad_clip_dev=clip["out"].data_ptr() if clip is not None else None,
                ema=ent["ema"].data_ptr() if decay is not None else None, ema_decay=decay if decay is not None else 0.0,
            )
            L.launch("grl_adamw_step", args)
            # the kernel wrote through raw pointers: tell autograd (and GRL's plan version stamp) that the tensors changed in place
            torch.autograd.graph.increment_version(plist)
        return loss
