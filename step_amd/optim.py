"""Fused clip_grad_norm_ + Adam for the native STEP module -- and for `TSFormer(mode="pre-train")` after `flatten_parameters()` -- (one pass over flat
buffers, libstep_hip).

Drop-in for the pair of torch calls the reference's training loop makes through easytorch
(``CFG.TRAIN.CLIP_GRAD_PARAM`` + ``CFG.TRAIN.OPTIM``, reference ``step/STEP_PEMS04.py:90-106``): same update
rule as ``torch.optim.Adam`` (L2 weight decay folded into the gradient, bias-corrected moments, eps added
after the square root) preceded by ``torch.nn.utils.clip_grad_norm_``.  Parameters that receive no gradient
(the reference leaves them at ``grad=None``, so torch's Adam skips them) are not part of the flat buffer.

It consumes the flat gradient buffer of the native backward (``model._flat_grad``): one backward per ``step()``, as in the
reference's loop -- or, after ``model.set_grad_accumulation(k)``, exactly ``k`` backwards whose gradients the native backward summed
in that buffer (the step count, bias correction and a scheduler advance per ``step()``, not per micro-batch).  Any other
accumulation over several backwards needs ``torch.optim.Adam`` on ``model.parameters()`` (``bench.py --torch-optim``), which reads
the accumulated ``.grad`` tensors.

Checkpoints: ``state_dict()`` / ``load_state_dict()`` speak ``torch.optim.Adam``'s format (one ``{"step", "exp_avg", "exp_avg_sq"}``
entry per parameter, indexed by the parameter's POSITION in the sequence ``params``), so a checkpoint written around either optimizer
resumes around the other.  The two conversions are the plain functions ``moments_to_state`` / ``state_to_moments`` below (no library,
no device needed).  With the graph learner in time slices the flat buffers hold one rank's columns of ``fc.weight``:
``FusedAdamClip(gathered_state=True)`` cuts a loaded state to them and emits torch's format after ``gather_state()``, a collective.
"""
import torch

from . import _lib
from .step_arch.discrete_graph_learning import cut_time_columns, paste_time_columns


def flat_items(model):
    """[(name, offset in floats, Parameter)] of the model's flat buffer, in buffer order: ``STEP._grad_layout()["items"]``, or the
    ``_pt_names`` of a pre-training ``TSFormer`` (every parameter starts at a multiple of four floats)"""
    if hasattr(model, "_pt_params"):
        items, off = [], 0
        for n, p in zip(model._pt_names, model._pt_params()):
            items.append((n, off, p))
            off += (p.numel() + 3) & ~3
        return items
    lay, tr = model._grad_layout(), dict(model._trainable())
    return [(k, lay["items"][k][0], tr[k]) for k in lay["order"]]


def index_flat_items(items, params, names=None):
    """-> ({position in ``params``: (name, offset, Parameter)}, {position: name} of every entry of ``params``).  Parameters are matched
    by identity; ``names`` maps id(Parameter) -> a name for the messages about parameters outside the flat buffer."""
    params = list(params)
    pos = {}
    for i, p in enumerate(params):
        pos.setdefault(id(p), i)
    missing = [n for n, _, p in items if id(p) not in pos]
    if missing:
        raise ValueError(f"FusedAdamClip: params lacks {len(missing)} parameter(s) of the flat buffer (first: {missing[0]!r}): pass every "
                         "parameter the native backward gives a gradient, in the order torch.optim.Adam would hold them")
    index = {pos[id(p)]: (n, off, p) for n, off, p in items}
    label = {i: index[i][0] if i in index else (names or {}).get(id(p), f"params[{i}]") for i, p in enumerate(params)}
    return index, label


def moments_to_state(index, exp_avg, exp_avg_sq, step, gathered=None):
    """flat moment buffers -> the ``"state"`` of ``torch.optim.Adam.state_dict()``: per flat parameter two VIEWS into the buffers (no
    copy, no synchronisation; ``torch.save`` writes the shared storage once) and ``step`` as torch keeps it, a 0-d float32 host tensor
    of its own.  Empty before the first step, as torch's.  ``gathered``: ``{position: (exp_avg, exp_avg_sq)}`` in the parameter's
    full shape for the positions of which the flat buffers hold only this rank's time slice (``FusedAdamClip.gather_state``)."""
    if int(step) == 0:
        return {}
    state = {}
    for i in sorted(index):
        _, off, p = index[i]
        n = p.numel()
        if gathered is not None and i in gathered:
            m, v = gathered[i]
        else:
            m, v = exp_avg[off:off + n].view(p.shape), exp_avg_sq[off:off + n].view(p.shape)
        state[i] = {"step": torch.tensor(float(step), dtype=torch.float32), "exp_avg": m, "exp_avg_sq": v}
    return state


def _step_value(v):
    v = float(v)          # an int, a float or a tensor on any device
    if v != int(v) or v < 0:
        raise ValueError(f"FusedAdamClip: step {v!r} in the optimizer state is not a step count")
    return int(v)


def state_to_moments(index, label, sd, exp_avg, exp_avg_sq, sliced=None):
    """``torch.optim.Adam.state_dict()`` -> the flat moment buffers (everything outside the parameters -- padding, spare slots -- is
    left zero); returns the common step count.  Saved parameter ids are mapped to positions the way ``Optimizer.load_state_dict`` does:
    in the order the groups list them.  Everything is checked before anything is written.  ``sliced``: ``{position: (T2, a, b)}`` for
    the positions of which the flat buffers hold only the time columns [a, b) (``cut_time_columns``): their moments arrive in the
    parameter's full shape, are checked against it, and this rank's columns are copied."""
    sliced = sliced or {}

    def extent(i):          # (offset, floats) of position i in the flat buffers
        _, off, p = index[i]
        if i in sliced:
            T2, a, b = sliced[i]
            return off, p.numel() // T2 * (b - a)
        return off, p.numel()
    ids = [i for g in sd["param_groups"] for i in g["params"]]
    if len(ids) != len(label):
        raise ValueError(f"FusedAdamClip: the optimizer state was saved around {len(ids)} parameters, this optimizer was given {len(label)}")
    position = {k: i for i, k in enumerate(ids)}
    entries, steps = {}, {}
    for k, st in sd["state"].items():
        if k not in position:
            raise ValueError(f"FusedAdamClip: state entry {k!r} belongs to no parameter of the saved groups")
        i = position[k]
        if i not in index:
            raise ValueError(f"FusedAdamClip: the optimizer state has an entry for {label[i]!r} (params[{i}]), which is not in the flat "
                             "buffer (frozen, or never given a gradient by the native backward)")
        name, off, p = index[i]
        for key in ("exp_avg", "exp_avg_sq"):
            if tuple(st[key].shape) != tuple(p.shape):
                raise ValueError(f"FusedAdamClip: {key} of {name!r} (params[{i}]) has shape {tuple(st[key].shape)}, the parameter "
                                 f"{tuple(p.shape)}")
        entries[i] = st
        steps[i] = _step_value(st["step"])
    if entries and len(entries) != len(index):
        lacking = [index[i][0] for i in sorted(index) if i not in entries]
        raise ValueError(f"FusedAdamClip: the optimizer state has entries for {len(entries)} of the {len(index)} parameters of the flat "
                         f"buffer (none for {lacking[0]!r}): the fused pass steps all of them together")
    if len(set(steps.values())) > 1:
        lo, hi = min(steps, key=steps.get), max(steps, key=steps.get)
        raise ValueError(f"FusedAdamClip: {index[lo][0]!r} is at step {steps[lo]}, {index[hi][0]!r} at step {steps[hi]}: the fused pass "
                         "keeps one step count for all parameters")
    if not entries:
        exp_avg.zero_()
        exp_avg_sq.zero_()
        return 0
    end = 0          # (the entries may be views of these very buffers -- load_state_dict(state_dict()) -- so only the gaps are zeroed)
    for off, n in sorted(extent(i) for i in index):
        exp_avg[end:off].zero_()
        exp_avg_sq[end:off].zero_()
        end = off + n
    exp_avg[end:].zero_()
    exp_avg_sq[end:].zero_()
    for i, st in entries.items():
        _, _, p = index[i]
        off, n = extent(i)
        if i in sliced:
            T2, a, b = sliced[i]
            exp_avg[off:off + n].view(p.shape[0], -1).copy_(cut_time_columns(st["exp_avg"].contiguous(), T2, a, b))
            exp_avg_sq[off:off + n].view(p.shape[0], -1).copy_(cut_time_columns(st["exp_avg_sq"].contiguous(), T2, a, b))
            continue
        exp_avg[off:off + n].view(p.shape).copy_(st["exp_avg"])
        exp_avg_sq[off:off + n].view(p.shape).copy_(st["exp_avg_sq"])
    return next(iter(steps.values()))


_ADAM_DEFAULTS = None


def adam_group(group, num_params):
    """a ``param_groups`` entry as ``torch.optim.Adam`` of THIS torch writes it: every key of its defaults (read from a live instance),
    overridden by ours (``lr``, ``betas``, ``eps``, ``weight_decay``, a scheduler's ``initial_lr``, ...), over positions 0 .. n - 1"""
    global _ADAM_DEFAULTS
    if _ADAM_DEFAULTS is None:
        _ADAM_DEFAULTS = dict(torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))]).defaults)
    out = dict(_ADAM_DEFAULTS)
    out.update({k: v for k, v in group.items() if k != "params"})
    out["params"] = list(range(num_params))
    return out


class FusedAdamClip(torch.optim.Optimizer):
    """A ``torch.optim.Optimizer`` (so ``torch.optim.lr_scheduler.MultiStepLR`` -- the reference's ``CFG.TRAIN.LR_SCHEDULER``,
    step/STEP_PEMS04.py:98-102 -- drives ``param_groups[0]["lr"]`` as usual) whose single parameter is the model's flat buffer."""

    # a HostFused-style subclass that skips __init__ (tests) is an optimizer without slices
    gathered_state = False
    _sliced = None          # {position of fc.weight in params: (T2, a, b)} while ``gathered_state`` acts
    _staging = None          # what gather_state() left: None, or {position: (exp_avg, exp_avg_sq)} (empty on the other ranks)

    def __init__(self, model, lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=None, param_grads=True, params=None,
                 gathered_state=False):
        """``param_grads=False`` (STEP only): the native backward leaves the gradients in the flat buffer this optimizer reads and does
        not hand ~100 per-parameter ``.grad`` views to autograd (0.3-0.5 ms of host time per step); ``p.grad`` stays None.
        ``params``: the ordered sequence of Parameters whose POSITIONS are the indices of ``state_dict()`` -- what the
        ``torch.optim.Adam`` this optimizer stands in for holds, or would hold (default: ``list(model.parameters())``).  Every
        parameter of the flat buffer must be in it (``ValueError``); matching is by identity, which flattening keeps.
        ``gathered_state`` (only with a graph learner in time slices, ignored otherwise): ``state_dict()`` / ``load_state_dict()``
        speak torch's format there too -- the flat buffer's ``fc.weight`` slice is bound to ``fc.weight``'s position in ``params``,
        a loaded state's full moments are cut to this rank's columns, and an emitted state takes ``fc.weight``'s full moments from
        ``gather_state()``, a collective.  Without it a sliced optimizer keeps the flat per-rank format (see ``state_dict``)."""
        self.model = model
        self.gathered_state = bool(gathered_state)
        if not param_grads and hasattr(model, "flat_gradients_only"):
            model.flat_gradients_only = True
        self.flat = model._flat_param if model._flat_param is not None else model.flatten_parameters()
        super().__init__([self.flat], dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.exp_avg = torch.zeros_like(self.flat)
        self.exp_avg_sq = torch.zeros_like(self.flat)
        self.max_norm = max_norm
        self.step_count = 0
        self.work = torch.empty(int(_lib.lib().step_adam_work_floats()), device=self.flat.device)
        self.grad_norm = torch.zeros(1, device=self.flat.device)
        self.dyn = None                     # device StepDynState while a GraphedTrainStep drives this optimizer
        model._backward_count = 0
        self._bind_params(params)

    def _sharded(self):
        return getattr(getattr(self.model, "discrete_graph_learning", None), "_shard", None) is not None

    def _bind_params(self, params):
        """the identity map between positions in ``params`` and the flat buffer.  With a sharded graph learner: none (see state_dict)
        -- or, with ``gathered_state``, the same map with the flat item ``dgl.fc_w`` (this rank's ``fc_weight_slice``) bound to the
        position and the full shape of ``fc.weight``, which is what ``params`` -- the replaced Adam's list -- holds"""
        self._index = self._label = self._sliced = self._staging = None
        items = flat_items(self.model)
        if self._sharded():
            if not self.gathered_state:
                return
            dgl = self.model.discrete_graph_learning
            items = [(n, off, dgl.fc.weight if n == "dgl.fc_w" else p) for n, off, p in items]
        params = list(self.model.parameters()) if params is None else list(params)
        names = {id(p): n for n, p in self.model.named_parameters()}
        self._index, self._label = index_flat_items(items, params, names)
        if self._sharded():
            sh = dgl._shard
            at = next(i for i, (n, _, _) in self._index.items() if n == "dgl.fc_w")
            self._sliced = {at: (dgl.train_length - 18, sh["a"], sh["b"])}

    def zero_grad(self, set_to_none=True):
        self.model.zero_grad(set_to_none=set_to_none)          # STEP.zero_grad also resets the flat-gradient bookkeeping

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise RuntimeError("FusedAdamClip.step() takes no closure")
        g = self.model._flat_grad
        if g is None:
            raise RuntimeError("FusedAdamClip.step(): no native backward has run since zero_grad()")
        k = getattr(self.model, "_grad_accum", 1)
        if k > 1 and self.dyn is not None:
            raise RuntimeError("FusedAdamClip.step(): gradient accumulation (k > 1) is not available while a GraphedTrainStep drives this optimizer")
        if k > 1 and self.model._backward_count != k:
            raise RuntimeError(f"FusedAdamClip.step(): {self.model._backward_count} native backwards since zero_grad(), the model accumulates "
                               f"{k} per step (set_grad_accumulation): the flat gradient buffer holds the sum of an unfinished group")
        if k == 1 and self.model._backward_count != 1:
            raise RuntimeError(f"FusedAdamClip.step(): {self.model._backward_count} native backwards since zero_grad() -- the flat gradient buffer "
                               "holds the last one only; accumulate with torch.optim.Adam on model.parameters() instead")
        if self.flat is not self.model._flat_param or g.numel() != self.flat.numel():
            # enable_native_data_parallel(shard_graph_learner=True) / flatten_parameters() after this optimizer was built re-home the
            # parameters: the captured buffer and moments no longer match the gradient layout
            raise RuntimeError("FusedAdamClip: the model's flat parameter buffer changed after the optimizer was created "
                               f"({self.flat.numel()} parameters here, {g.numel()} gradient values): build the optimizer after "
                               "enable_native_data_parallel() / flatten_parameters()")
        # Whatever averaged the gradients (DDP bucket views, a hand-written all-reduce over p.grad) must have acted on THIS buffer --
        # autograd clones a view that has another owner, DDP may swap in its own.  First, middle and last parameter are enough to tell
        # (the buffer is adopted or replaced as a whole).  Both the pre-training TSFormer and STEP hand out views of one flat buffer.
        ps = self.model._pt_params() if hasattr(self.model, "_pt_params") else self.model._trainable_list()
        lo, hi = g.data_ptr(), g.data_ptr() + g.numel() * g.element_size()
        for q in (ps[0], ps[len(ps) // 2], ps[-1]):
            if q.grad is not None and not (lo <= q.grad.data_ptr() < hi):
                raise RuntimeError("FusedAdamClip: a parameter's .grad is not a view of the native flat gradient buffer (cloned by autograd or "
                                   "re-homed by a DDP wrapper): reduce model._flat_grad itself, or step with torch.optim.Adam")
        pg = self.param_groups[0]
        self.step_count += 1
        self._staging = None          # (gather_state: the moments are about to change)
        if hasattr(self.model, "_drop_eval_g"):
            self.model._drop_eval_g()          # the kernel writes the parameters through raw pointers (no version bump): STEP's kept eval-mode g is stale
        extra = None
        max_norm = float(self.max_norm or 0.0)
        sh = getattr(getattr(self.model, "discrete_graph_learning", None), "_shard", None)      # (a TSFormer in pre-training mode has no graph learner)
        if sh is not None:
            # the fc weight slices of the other ranks belong to the model's gradient norm: the sum of their squared norms came back
            # in the layout's spare slot with the gradient all-reduce (step.py backward) -- no collective of its own
            extra = self.model._other_slices_sumsq
            if max_norm > 0.0 and self.dyn is None and getattr(self.model, "_total_sumsq", None) is not None:
                # ... as the whole squared norm, formed identically on every rank (step.py backward): max_norm < 0 tells the kernel to take
                # it as is.  Only with a real threshold: -0.0 is not "< 0" for the kernel, which would then add its own sum to the total
                extra, max_norm = self.model._total_sumsq, -max_norm
        if self.dyn is not None:
            # replayed (graph-captured) step: the step count and the learning rate are read from the device state (step_amd/graphed.py
            # advances the count at the head of every replay and copies the scheduler's rate when it changes)
            _lib.call("step_adam_clip_dyn", _lib.ptr(self.flat), _lib.ptr(g), _lib.ptr(self.exp_avg), _lib.ptr(self.exp_avg_sq),
                      self.flat.numel(), float(pg["betas"][0]), float(pg["betas"][1]), float(pg["eps"]), float(pg["weight_decay"]),
                      float(self.max_norm or 0.0), _lib.ptr(extra), _lib.ptr(self.work), _lib.ptr(self.grad_norm), _lib.ptr(self.dyn),
                      _lib.stream())
            return
        _lib.call("step_adam_clip_sharded", _lib.ptr(self.flat), _lib.ptr(g), _lib.ptr(self.exp_avg), _lib.ptr(self.exp_avg_sq),
                  self.flat.numel(), float(pg["lr"]), float(pg["betas"][0]), float(pg["betas"][1]), float(pg["eps"]),
                  float(pg["weight_decay"]), self.step_count, max_norm, _lib.ptr(extra), _lib.ptr(self.work),
                  _lib.ptr(self.grad_norm), _lib.stream())

    def state_dict(self):
        """``torch.optim.Adam``'s format over the constructor's ``params``: ``{"state": {position: {"step", "exp_avg", "exp_avg_sq"}},
        "param_groups": [...]}``, one entry per parameter of the flat buffer (none for frozen ones, none at all before the first step).
        The moments are views into the flat buffers, live like the tensors of torch's own ``state_dict()``: a ``torch.optim.Adam``
        over the same parameter sequence loads the result (``copy.deepcopy`` it first if both optimizers go on stepping).
        While a ``GraphedTrainStep`` is attached the step count is on the device: ``close()`` it first.
        With a sharded graph learner (``discrete_graph_learning._shard``) the flat buffer holds this rank's ``fc.weight`` slice, which
        is no parameter of torch's format: there both methods keep the flat per-rank format ``{"step", "exp_avg", "exp_avg_sq",
        "param_groups"}`` (one file per rank) -- unless the optimizer was built with ``gathered_state=True``: then it is torch's format
        here too, ``fc.weight``'s entry holding the full moments that ``gather_state()`` assembled on the group's rank 0.  Once a step
        has run, a ``state_dict()`` without a gather since the last step -- or on another rank than the one that holds the gathered
        moments -- raises ``RuntimeError``: one rank's slice is never written as if it were the whole."""
        if self._index is None:
            groups = [{k: v for k, v in g.items() if k != "params"} for g in self.param_groups]
            return {"step": self.step_count, "exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq, "param_groups": groups}
        gathered = None
        if self._sliced is not None and self.step_count > 0:
            gathered = self._staging
            if gathered is None:
                raise RuntimeError("FusedAdamClip: the graph learner is sharded in time slices and this optimizer has stepped since the "
                                   "last gather: call gather_state() on ALL ranks (e.g. in the runner's on_epoch_end) before "
                                   "state_dict() -- the flat buffers hold the moments of this rank's fc.weight slice only")
            if sorted(gathered) != sorted(self._sliced):
                raise RuntimeError("FusedAdamClip: gather_state() assembled fc.weight's moments on the group's rank 0; this rank holds "
                                   "its slice only and has no complete state_dict() to give")
        return {"state": moments_to_state(self._index, self.exp_avg, self.exp_avg_sq, self.step_count, gathered),
                "param_groups": [adam_group(self.param_groups[0], len(self._label))]}

    def gather_state(self, process_group=None):
        """Collective (``gathered_state=True`` with a sharded graph learner; a no-op otherwise): assemble the full ``exp_avg`` /
        ``exp_avg_sq`` of ``fc.weight`` on the group's rank 0, in two staging tensors of ``fc.weight``'s shape, for ``state_dict()``.
        One broadcast per rank and moment, each of that rank's slice straight out of its flat buffer; a rank that is neither the
        sender nor rank 0 receives into a temporary of one slice.  The staging stays valid until the next ``step()``,
        ``load_state_dict()`` or ``release_state()``."""
        if self._sliced is None:
            return
        import torch.distributed as dist
        dgl = self.model.discrete_graph_learning
        sh = dgl._shard
        (at, (T2, _, _)), = self._sliced.items()
        _, off, p = self._index[at]
        root = sh["rank"] == 0
        staged = tuple(torch.empty(p.shape, dtype=buf.dtype, device=buf.device) for buf in (self.exp_avg, self.exp_avg_sq)) if root else ()
        for r in range(sh["world"]):
            a, b = sh["bounds"][r], sh["bounds"][r + 1]
            n = p.shape[0] * (p.shape[1] // T2) * (b - a)
            src = dist.get_global_rank(process_group, r) if process_group is not None else r
            for k, buf in enumerate((self.exp_avg, self.exp_avg_sq)):
                piece = buf[off:off + n] if r == sh["rank"] else torch.empty(n, dtype=buf.dtype, device=buf.device)
                if sh["world"] > 1:
                    dist.broadcast(piece, src, group=process_group)
                if root:
                    paste_time_columns(staged[k], T2, a, b, piece)
                del piece
        self._staging = {at: staged} if root else {}

    def release_state(self):
        """drop what ``gather_state()`` assembled (two tensors of ``fc.weight``'s size on rank 0)"""
        self._staging = None

    def load_state_dict(self, sd):
        """torch's format (see ``state_dict``; ``ValueError`` for a state the fused pass cannot hold: another shape, an entry for a
        parameter outside the flat buffer, entries for only some parameters, different step counts), or the flat format of
        checkpoints written before (``"exp_avg"`` as a top-level key).  With ``gathered_state=True`` over a sharded graph learner:
        torch's format with ``fc.weight``'s moments in the full shape, of which this rank keeps its columns -- no collective, every
        rank reads the same state."""
        if "exp_avg" in sd:
            self.step_count = _step_value(sd["step"])
            self.exp_avg.copy_(sd["exp_avg"])
            self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        elif self._index is None:
            raise ValueError("FusedAdamClip: with a sharded graph learner the optimizer state is the flat per-rank format, not torch's")
        else:
            self.step_count = state_to_moments(self._index, self._label, sd, self.exp_avg, self.exp_avg_sq, self._sliced)
        self._staging = None          # (after the copies: the loaded entries may be the staging's own tensors)
        for g, src in zip(self.param_groups, sd["param_groups"]):
            g.update({k: v for k, v in src.items() if k != "params"})
