"""The whole n_layer x (global, local) loop of PAMNet.forward (models.py:196-204) as ONE engine call per direction, at
every width an engine is built for: `pamnet_stack_*` dispatch on d inside the library (csrc/engine.hip at dim = 128,
csrc/narrow_engine.hip at dim = 16 / 32 / 64).  ~7 launches per layer pair forward, ~16 backward at dim = 128; the
reference issues ~150 per layer pair for the same work.
"""
import ctypes
import os

import torch

from . import lib, narrow
from .fused import D, _empty, _iarr, _parr, alloc_like_grouped, tail_params
from .ops import apply as _apply, direct_allowed


class StackCtx(object):
    """Per-model hand-over between a trainer and the layer-stack backward: `events` = n_layer torch.cuda.Event (already
    recorded once, so their handles exist) the engine records as each layer pair's gradients are enqueued -- the trainer
    overlaps the gradient all-reduce of the last layers with the backward of the first ones; `recorded` is set by the
    backward when it handed the events to the engine."""

    def __init__(self):
        self.events, self.recorded = None, False


def stack_ctx(global_layers):
    """The StackCtx of a model's layer stack (created on first use, stored on the global_layer ModuleList)."""
    ctx = getattr(global_layers, '_pamnet_ctx', None)
    if ctx is None:
        ctx = global_layers._pamnet_ctx = StackCtx()
    return ctx


def global_params(layer):      # slot order: csrc/common.h pslot::Global
    lin_m = layer.mlp_m[0][0]
    return [layer.mlp_x1[0][0].weight, layer.mlp_x1[0][0].bias, lin_m.weight, lin_m.bias,
            layer.W_edge_attr.weight] + tail_params(layer)


def local_params(layer):       # slot order: csrc/common.h pslot::Local
    lin_ji = layer.mlp_m_ji[0][0]
    lin_kj = (layer.mlp_m_jj if layer.small else layer.mlp_m_kj)[0][0]
    s1, s2 = layer.mlp_sbf[0][0], layer.mlp_sbf[1][0]
    return [layer.mlp_x1[0][0].weight, layer.mlp_x1[0][0].bias, lin_ji.weight, lin_ji.bias, lin_kj.weight,
            lin_kj.bias, s1.weight, s1.bias, s2.weight, s2.bias, layer.lin_rbf.weight,
            layer.lin_rbf_out.weight] + tail_params(layer)


_AUX = {}
PACK_WEIGHTS = os.environ.get('PAMNET_PACK_WEIGHTS', '1') != '0'
AUX_FORK = os.environ.get('PAMNET_AUX_FWD', '0') != '0'      # measured: no gain at B=128 (host-side event cost, CU contention)


def _aux_fork(dev, n_layer):
    """(aux stream handle, event handle array) for the forward's x-independent branch; (None, None) when disabled."""
    if not AUX_FORK:
        return None, None
    key = (dev, n_layer)
    if key not in _AUX:
        stream = torch.cuda.Stream(device=dev)
        events = [torch.cuda.Event() for _ in range(n_layer + 1)]
        for e in events:
            e.record(torch.cuda.current_stream(dev))      # materialise the handles
        _AUX[key] = (stream, events, _parr([int(e.cuda_event) for e in events]))
    stream, _, arr = _AUX[key]
    return stream.cuda_stream, arr


def _graph_tables(graph):
    t = getattr(graph, '_tables', None)        # a graph built by the graph-construction engine carries its tables
    if t is not None:
        return t
    sizes = _iarr([graph.n, graph.glob.m, graph.loc.m, graph.tp.m])
    idx = _parr([graph.glob.ptr, graph.glob.row_of, graph.glob.col, graph.glob_T.ptr, graph.glob_T.perm,
                 graph.loc.ptr, graph.loc.row_of, graph.loc.col, graph.loc_T.ptr, graph.loc_T.perm,
                 graph.tp.ptr, graph.tp.row_of, graph.tp.col, graph.tp_T.ptr, graph.tp_T.perm,
                 getattr(graph, 'seg_cuts', None), getattr(graph, 'tT_edge', None), getattr(graph, 'tT_node', None)])
    return sizes, idx


_data_ptr = torch.Tensor.data_ptr
_grad_of = torch.Tensor.grad.__get__


class StackPlan(object):
    """Parameter tables of a layer stack: walking the nn.Module tree (~400 attribute / Sequential lookups) costs ~0.5 ms of
    host time per step, comparable to enqueueing the kernels, so the Parameter OBJECTS are listed once and the list is kept
    for as long as the module tree holds exactly these objects (stack_plan).  What an object points at may change under the
    list (`p.data = t`, `model.to(...)`, a .grad set to None or replaced): the pointer arrays are keyed by the address of
    EVERY tensor they hold -- data_ptr() of each, once per engine call -- and rebuilt when any of them has moved (host cost
    against the three-tensor key this replaces: profiles/live_params_ab.txt).  `table_calls` counts param_tables() calls:
    a holder of the parameters (train.Trainer) tells from it whether a forward went through the engine and so refreshed
    `_pkey`."""

    def __init__(self, global_layers, local_layers):
        self.gl = [global_params(l) for l in global_layers]
        self.ll = [local_params(l) for l in local_layers]
        self.L = len(self.gl)
        self.d = self.gl[0][0].size(0)                     # mlp_x1.W [d, d]
        self.gflat = [p for lay in self.gl for p in lay]
        self.lflat = [p for lay in self.ll for p in lay]
        self.flat = self.gflat + self.lflat
        self._flag_probe = [self.flat[0], self.flat[len(self.flat) // 2], self.flat[-1]]
        self._pkey = self._gkey = None
        self.table_calls = 0
        self._shape_groups = None           # {(shape, dtype, device): [indices into self.flat]} for grouped gradient allocation
        self._pack = self._temp = None
        self.ctx = stack_ctx(global_layers)

    def temp_arena(self, n_floats, dev):
        """Scratch arena of this model's engine calls (stream-ordered use; grown on demand)."""
        t = self._temp
        if t is None or t.numel() < n_floats or t.device != dev:
            t = self._temp = torch.empty(int(n_floats * 1.25) + 1024, dtype=torch.float32, device=dev)
        return t

    def pack_arena(self, dev):
        """Scratch for the fragment-ordered weight images the node chains read (re-packed by every engine call)."""
        if not PACK_WEIGHTS:
            return None
        if self._pack is None or self._pack.device != dev:
            need = ctypes.c_int64(0)
            lib.call('pamnet_stack_pack_floats', self.L, self.d, ctypes.addressof(need))
            self._pack = torch.empty(int(need.value), dtype=torch.float32, device=dev)
        return self._pack

    def matches(self, global_layers, local_layers):
        """True when the two stacks hold, slot by slot, exactly the Parameter objects listed here (a full walk)."""
        if len(global_layers) != self.L or len(local_layers) != len(self.ll):
            return False
        try:
            live = [p for l in global_layers for p in global_params(l)] + [p for l in local_layers for p in local_params(l)]
        except (AttributeError, IndexError, TypeError):     # a layer of another kind was hung in
            return False
        return len(live) == len(self.flat) and all(a is b for a, b in zip(live, self.flat))

    def param_tables(self):
        self.table_calls += 1
        key = tuple(map(_data_ptr, self.flat))
        if key != self._pkey:
            ng = len(self.gflat)
            self._gtab, self._ltab = _parr(key[:ng]), _parr(key[ng:])
            self._pkey = key
        return self._gtab, self._ltab

    def direct(self):
        """True when every parameter owns a preallocated contiguous .grad handed out by train.FlatParams (which zeroes
        it every step: direct writes overwrite, they do not accumulate) with direct writes allowed.  The gradient tables
        are keyed by the address of every .grad: one that was dropped or replaced since they were built is seen."""
        # (FlatParams.set_direct flips the permission of all parameters at once: three of them tell)
        if not all(getattr(p, '_pamnet_direct', False) for p in self._flag_probe):
            return False
        try:
            key = tuple(map(_data_ptr, map(_grad_of, self.flat)))
        except TypeError:                                   # a .grad is None
            return False
        if key != self._gkey:
            if not all(getattr(p, '_pamnet_direct', False) and p.grad.is_contiguous() for p in self.flat):
                return False
            ng = len(self.gflat)
            self._ggrad, self._lgrad = _parr(key[:ng]), _parr(key[ng:])
            self._gkey = key
        return True


class _Stack(torch.autograd.Function):
    """x0, e_g, rbf_e, e_sbf -> outs [2L,N], atts [2L,N] (and the saved-activation arena).  One C call forward, one
    backward.  In direct-gradient mode the parameters are not autograd inputs (their gradients are written straight into
    the flat buffer): ~400 fewer edges for the autograd engine to walk."""

    @staticmethod
    def forward(ctx, x0, e_g, rbf_e, e_sbf, graph, plan, direct, save, *params):
        x0, e_g, rbf_e, e_sbf = x0.contiguous(), e_g.contiguous(), rbf_e.contiguous(), e_sbf.contiguous()
        L, (n, d) = plan.L, x0.shape
        sizes, idx = _graph_tables(graph)
        need = (ctypes.c_int64 * 2)()
        lib.call('pamnet_stack_workspace', n, e_g.size(0), rbf_e.size(0), e_sbf.size(0), L, d,
                 ctypes.addressof(need), ctypes.addressof(need) + 8)
        saved = torch.empty(max(int(need[0]), 1), dtype=torch.float32, device=x0.device)
        temp = plan.temp_arena(int(need[1]), x0.device)
        outs, atts = _empty(2 * L, n, like=x0), _empty(2 * L, n, like=x0)
        gtab, ltab = plan.param_tables()
        aux, evs = _aux_fork(x0.device, L)
        lib.call('pamnet_stack_fwd_f32', sizes, idx, L, d, lib.ptr(x0), lib.ptr(e_g), lib.ptr(rbf_e), lib.ptr(e_sbf),
                 gtab, ltab, lib.ptr(saved), lib.ptr(temp), lib.ptr(outs), lib.ptr(atts),
                 1 if save else 0, lib.ptr(plan.pack_arena(x0.device)), aux, evs, lib.stream_of(x0))
        ctx.save_for_backward(x0, e_g, rbf_e, e_sbf, saved)
        ctx.graph, ctx.plan, ctx.direct, ctx.temp_floats = graph, plan, direct, int(need[1])
        ctx.pkey, ctx.gkey = plan._pkey, plan._gkey if direct else None
        ctx.mark_non_differentiable(saved)
        ctx.set_materialize_grads(False)       # else autograd zero-fills a gradient the size of `saved` every step
        return outs, atts, saved

    @staticmethod
    def backward(ctx, g_outs, g_atts, _g_saved):
        x0, e_g, rbf_e, e_sbf, saved = ctx.saved_tensors
        graph, plan, direct = ctx.graph, ctx.plan, ctx.direct
        L, (n, d) = plan.L, x0.shape
        sizes, idx = _graph_tables(graph)
        temp = plan.temp_arena(ctx.temp_floats, x0.device)
        d_x0, d_eg, d_rbf, d_sbf = (torch.empty_like(t) for t in (x0, e_g, rbf_e, e_sbf))
        gtab, ltab = plan.param_tables()
        # The saved activations belong to the weights the forward read, and in direct mode the gradients go where the
        # forward's table says: a tensor re-pointed (`p.data = t`, a device move) or a .grad replaced between a forward
        # and its backward would mix the two silently -- refused before anything is launched.  (Keys are rebuilt only
        # when an address changed: identity is enough.)
        if plan._pkey is not ctx.pkey or (direct and plan._gkey is not ctx.gkey):
            raise RuntimeError('PAMNet layer stack: a parameter tensor (or, with direct gradient writes, a .grad) was '
                               're-pointed or moved between this forward and its backward; the backward cannot '
                               'differentiate the forward that ran. Run the forward again after the edit.')
        evs = None
        if direct:
            ggrad, lgrad, g = plan._ggrad, plan._lgrad, ()
            sc = plan.ctx
            if sc.events is not None and len(sc.events) == L:
                evs = _parr([int(e.cuda_event) for e in sc.events])
                sc.recorded = True
        else:
            if plan._shape_groups is None or next(iter(plan._shape_groups))[2] != plan.flat[0].device:
                plan._shape_groups = {}                        # (first use, or the model moved)
                for i, p in enumerate(plan.flat):
                    plan._shape_groups.setdefault((tuple(p.shape), p.dtype, p.device), []).append(i)
            g, ptrs = alloc_like_grouped(plan.flat, plan._shape_groups)
            ng = len(plan.gflat)
            ggrad, lgrad = (ctypes.c_void_p * ng)(*ptrs[:ng]), (ctypes.c_void_p * (len(ptrs) - ng))(*ptrs[ng:])
        g_outs = torch.zeros(2 * L, n, device=x0.device) if g_outs is None else g_outs.contiguous()
        g_atts = torch.zeros_like(g_outs) if g_atts is None else g_atts.contiguous()
        lib.call('pamnet_stack_bwd_f32', sizes, idx, L, d, lib.ptr(x0), lib.ptr(e_g), lib.ptr(rbf_e), lib.ptr(e_sbf),
                 gtab, ltab, lib.ptr(saved), lib.ptr(temp), lib.ptr(g_outs), lib.ptr(g_atts), ggrad, lgrad,
                 lib.ptr(d_x0), lib.ptr(d_eg), lib.ptr(d_rbf), lib.ptr(d_sbf), lib.ptr(plan.pack_arena(x0.device)), evs,
                 lib.stream_of(x0))
        return (d_x0, d_eg, d_rbf, d_sbf, None, None, None, None) + tuple(g)


def stack_plan(global_layers, local_layers, checked=False):
    """The StackPlan of a model's layer stack (stored on the global_layer ModuleList).  It lists Parameter objects, so it
    holds only while the two stacks hold exactly those objects: a replaced head module, a Parameter assigned over another,
    `load_state_dict(..., assign=True)` or a replaced layer make it stale.  `checked=True`: the caller vouches for that --
    models.PAMNet validates its cached parameter walk against the live module tree once per forward and drops the plan
    together with the walk (drop_plan), so the engine call inside that forward repeats nothing.  Every other caller
    pays the walk here."""
    plan = getattr(global_layers, '_pamnet_plan', None)
    if plan is not None and not checked and not plan.matches(global_layers, local_layers):
        plan = None
    if plan is None or plan.L != len(global_layers):
        plan = StackPlan(global_layers, local_layers)
        global_layers._pamnet_plan = plan
    return plan


def drop_plan(global_layers):
    """Forget the plan of a layer stack whose owner has seen (or made) a change to the module tree."""
    if global_layers is not None:
        global_layers.__dict__.pop('_pamnet_plan', None)


def engine_supported(x, graph):
    """dim = 128 on an MI355X always takes the engine; dim = 16 / 32 / 64 under narrow.engine_supported's conditions."""
    return (x.is_cuda and x.size(-1) == D) or narrow.engine_supported(x, graph)


def layer_stack(global_layers, local_layers, x0, e_g, rbf_e, e_sbf, graph, tape=None, checked=False):
    """Returns outs [2L,N], atts [2L,N] and the saved-activation arena (see stack_x_layers).  `checked`: see stack_plan."""
    plan = stack_plan(global_layers, local_layers, checked)
    # inference (no gradient mode): the engine skips every store only the backward would read
    save = torch.is_grad_enabled()
    if tape is not None:                       # direct-gradient mode on the model's own tape (ops.Tape)
        return tape.call(_Stack, x0, e_g, rbf_e, e_sbf, graph, plan, True, True)
    if save and direct_allowed() and plan.direct():
        return _Stack.apply(x0, e_g, rbf_e, e_sbf, graph, plan, True, True)
    if not save:
        # forward-only: no autograd node (handing ~400 parameters to Function.apply costs ~0.1 ms of host time per
        # batch -- the forward-only loop is bound by the host, not by the 0.8 ms of kernels)
        return _apply(_Stack, x0, e_g, rbf_e, e_sbf, graph, plan, False, False)
    return _Stack.apply(x0, e_g, rbf_e, e_sbf, graph, plan, False, save, *plan.flat)


def stack_x_layers(saved, graph, n_layer, d):
    """Node features after every layer (global_0, local_0, ...) as views into the saved arena."""
    lay = (ctypes.c_int64 * 3)()
    lib.call('pamnet_stack_layout', graph.n, graph.glob.m, graph.loc.m, graph.tp.m, d, ctypes.addressof(lay))
    pair, og, ol = int(lay[0]), int(lay[1]), int(lay[2])
    n = graph.n
    xs = []
    for k in range(n_layer):
        for off in (og, ol):
            xs.append(saved[k * pair + off:k * pair + off + n * d].view(n, d))
    return xs
