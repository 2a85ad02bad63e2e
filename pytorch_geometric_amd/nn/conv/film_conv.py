import copy
import os
import weakref
from typing import Callable, Optional, Tuple, Union

import torch
from torch import Tensor
from torch.nn import Linear, ModuleList, ReLU

from ... import _native
from ..._functions import FiLMAggregateFunction, linear
from ..._onepass import FilmForms
from ...edge_index import EdgeIndex
from .gmm_conv import device_floats, stock_flow
from .message_passing import _LOW, MessagePassing, _n_dst

# PYGAMD_FUSE_FILM: whether a FiLMConv starts with ``fuse = True`` (read at import).  The default
# is 1 because the fused training step was measured faster than the generic one at all three
# shapes of profiles/film_conv.md: 3.6 against 10.3 ms (R = 1, F = 320), 6.5 against 28.5 ms
# (R = 4, F = 128) and 6.8 against 45.8 ms (R = 16, F = 64).
_DEFAULT_FUSE_FILM = '1'
FUSE_FILM = os.environ.get('PYGAMD_FUSE_FILM', _DEFAULT_FUSE_FILM).strip() not in ('', '0')


def _reset(module):
    """``torch_geometric.nn.inits.reset``: every ``reset_parameters`` below ``module``"""
    if hasattr(module, 'reset_parameters'):
        module.reset_parameters()
    else:
        for child in (module.children() if hasattr(module, 'children') else []):
            _reset(child)


class FiLMConv(MessagePassing):
    r"""The feature-wise linear modulation operator (GNN-FiLM) with the constructor arguments,
    state-dict keys (``lins.{r}.weight``, ``films.{r}.*``, ``lin_skip.weight``, ``film_skip.*``),
    ``__repr__`` and forward semantics of ``torch_geometric.nn.FiLMConv``
    (torch_geometric/nn/conv/film_conv.py:19-165):

    .. math:: x_i' = \mathrm{act}(\gamma^s_i \odot W_s x_i + \beta^s_i) + \sum_r
        \mathrm{aggr}_{j \in N_r(i)} \mathrm{act}(\gamma_{r,i} \odot W_r x_j + \beta_{r,i}),
        \quad [\beta_{r,i} | \gamma_{r,i}] = \mathrm{film}_r(x_i)

    ``in_channels`` is an int or a ``(src, dst)`` pair, ``x`` a tensor or a ``(x_src, x_dst)``
    pair.  A caller's ``nn`` (node features -> ``2 * out_channels``) is deep-copied per relation
    and for the skip term; the default is ``Linear`` (the skip's without bias).  Routes:

    * fused (device tensors, float32 after widening, ``fuse`` true, ``flow='source_to_target'``,
      ``aggr`` in add / sum / mean, ``act`` None or exactly a ``torch.nn.ReLU``, ``out_channels
      <= 512``): the ``R`` source transforms are ONE dense product ``H = x_src @ [W_0 ; ...]^T``
      and, with the default film nets, the ``R`` modulations one more, ``G = [film_0(x_dst) | ...]``
      — with one ``x`` in both roles ONE ``[N, 3 R F]`` plane ``[H | G]``, whose gradient is one
      plane.  A caller's ``nn`` runs on the nodes and its ``R`` outputs are concatenated.  All
      relations then take ONE kernel forward and two backward (``FiLMAggregateFunction``,
      csrc/film.hip) that gather one ``F`` row per edge, keep ``[beta | gamma]`` of the current
      relation in registers and recompute the activation in the backward: nothing of size ``E x
      F`` is formed or saved.  The skip term is node-level torch code on a second stacked product
      and rides in the kernel's epilogue.  The edges are sorted by relation, then by destination,
      once per ``(edge_index, edge_type)`` pair (cached on the layer by tensor identity and
      version, with the two pair handles of the backward and the mean normaliser);
    * the reference's loop of one masked ``propagate`` per relation for everything else (host
      tensors, float64, ``fuse = False``, ``target_to_source``, ``max`` and other aggregations,
      another ``act``, ``out_channels > 512``) — and whenever the message flow is observed or
      replaced: a propagate, message or aggregate hook, explain mode, or a subclass with its own
      ``message``, ``aggregate``, ``update`` or ``propagate``.

    With ``num_relations <= 1`` ``edge_type`` is ignored; with more it is required
    (``ValueError``).  Edges whose type lies outside ``[0, num_relations)`` contribute nothing on
    either route (no mask of the reference's loop selects them).  Half and bfloat16 device inputs
    are widened to float32 and the result handed back in their dtype outside autocast.  ``fuse``
    is a per-layer attribute initialised from the environment switch ``PYGAMD_FUSE_FILM`` (read
    at import)."""

    def __init__(self, in_channels: Union[int, Tuple[int, int]], out_channels: int,
                 num_relations: int = 1, nn: Optional[Callable] = None,
                 act: Optional[Callable] = ReLU(), aggr: str = 'mean', **kwargs):
        super().__init__(aggr=aggr, **kwargs)
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.num_relations = max(num_relations, 1)
        self.act = act
        if isinstance(in_channels, int):
            in_channels = (in_channels, in_channels)
        self.lins = ModuleList()
        self.films = ModuleList()
        for _ in range(num_relations):
            self.lins.append(Linear(in_channels[0], out_channels, bias=False))
            self.films.append(Linear(in_channels[1], 2 * out_channels) if nn is None
                              else copy.deepcopy(nn))
        self.lin_skip = Linear(in_channels[1], out_channels, bias=False)
        self.film_skip = (Linear(in_channels[1], 2 * out_channels, bias=False) if nn is None
                          else copy.deepcopy(nn))
        self._default_nn = nn is None
        self._widths = (int(in_channels[0]), int(in_channels[1]))
        self.fuse = FUSE_FILM
        self.reset_parameters()

    def reset_parameters(self):
        super().reset_parameters()
        for lin, film in zip(self.lins, self.films):
            lin.reset_parameters()
            _reset(film)
        self.lin_skip.reset_parameters()
        _reset(self.film_skip)

    def _fusable(self, x_src, x_dst) -> bool:
        if not stock_flow(self, FiLMConv):
            return False
        return bool(self.fuse and self.flow == 'source_to_target'
                    and self.aggr in ('add', 'sum', 'mean')
                    and (self.act is None or type(self.act) is ReLU)
                    and device_floats(x_src, x_dst)
                    and x_src.size(1) == self._widths[0] and x_dst.size(1) == self._widths[1]
                    and self.out_channels <= 512 and len(self.lins) == self.num_relations)

    def forward(self, x: Union[Tensor, Tuple[Tensor, Tensor]], edge_index,
                edge_type: Optional[Tensor] = None) -> Tensor:
        if isinstance(x, Tensor):
            x = (x, x)
        if self.num_relations > 1 and edge_type is None:
            raise ValueError(f"'edge_type' is required with num_relations = "
                             f"{self.num_relations}")
        if self._fusable(x[0], x[1]):
            return self._forward_fused(x[0], x[1], edge_index, edge_type)
        F = self.out_channels
        beta, gamma = self.film_skip(x[1]).split(F, dim=-1)
        out = gamma * self.lin_skip(x[1]) + beta
        if self.act is not None:
            out = self.act(out)
        if self.num_relations <= 1:
            beta, gamma = self.films[0](x[1]).split(F, dim=-1)
            return out + self.propagate(edge_index, x=self.lins[0](x[0]), beta=beta, gamma=gamma)
        ei, size = edge_index, None
        if isinstance(edge_index, EdgeIndex):  # (a masked copy keeps the handle's sizes)
            ei, size = edge_index.edge_index, edge_index.sparse_size
        for i, (lin, film) in enumerate(zip(self.lins, self.films)):
            beta, gamma = film(x[1]).split(F, dim=-1)
            mask = edge_type == i
            out = out + self.propagate(ei[:, mask], size=size, x=lin(x[0]), beta=beta,
                                       gamma=gamma)
        return out

    def _forms(self, ei: Tensor, edge_type: Optional[Tensor], n_src: int, n_dst: int) -> FilmForms:
        """The layer's sorted forms for this ``(edge_index, edge_type)`` pair, cached by tensor
        identity + in-place version: one sort by relation, one by destination and the two pair
        sorts per graph, not per call."""
        typed = self.num_relations > 1
        et = edge_type if typed else None
        mean = self.aggr == 'mean'
        hit = self.__dict__.get('_film_cache')
        if hit is not None:
            r_ei, r_et, v_ei, v_et, key, forms = hit
            if (r_ei() is ei and v_ei == ei._version and key == (n_src, n_dst, mean)
                    and (r_et() if r_et is not None else None) is et
                    and v_et == (et._version if et is not None else None)):
                return forms
        forms = self._build_forms(ei, et, n_src, n_dst, mean)
        self.__dict__['_film_cache'] = (
            weakref.ref(ei), None if et is None else weakref.ref(et), ei._version,
            None if et is None else et._version, (n_src, n_dst, mean), forms)
        return forms

    def _build_forms(self, ei, et, n_src, n_dst, mean) -> FilmForms:
        R = self.num_relations
        src, dst = ei[0], ei[1]
        E = src.numel()
        if et is None:
            rel = torch.zeros(E, dtype=torch.int32, device=ei.device)
        else:
            if et.dim() != 1 or et.numel() != E:
                raise ValueError(f"'edge_type' must hold one entry per edge (got "
                                 f"{tuple(et.shape)} for {E} edges)")
            et = et.to(torch.int64)
            if E > 0:
                lo, hi = _native.index_minmax(et)
                if lo < 0 or hi >= R:
                    # no mask `edge_type == r` of the reference's loop selects these edges
                    keep = (et >= 0) & (et < R)
                    src, dst, et = src[keep], dst[keep], et[keep]
            # by relation first: the stable by-destination sort then groups every row by relation
            _, perm = _native.index_sort(et, max_value=R - 1)
            src, dst, rel = src[perm], dst[perm], et[perm].to(torch.int32)
        return FilmForms.of_edges(src.contiguous(), dst.contiguous(), rel, n_src, n_dst, R, mean)

    def _forward_fused(self, x_src: Tensor, x_dst: Tensor, edge_index,
                       edge_type: Optional[Tensor]) -> Tensor:
        F, R = self.out_channels, self.num_relations
        low = x_src.dtype if x_src.dtype in _LOW else None
        xs = x_src.float()
        xd = xs if x_dst is x_src else x_dst.float()
        n_dst = _n_dst(self, x_src, x_dst, edge_index, None)
        n_src = edge_index.num_src_nodes if isinstance(edge_index, EdgeIndex) else xs.size(0)
        ei = edge_index.edge_index if isinstance(edge_index, EdgeIndex) else edge_index
        forms = self._forms(ei, edge_type, n_src, n_dst)
        with torch.autocast('cuda', enabled=False):
            w_h = torch.cat([lin.weight.float() for lin in self.lins])          # [R F, F_src]
            if self._default_nn:
                w_g = torch.cat([film.weight.float() for film in self.films])   # [R 2F, F_dst]
                b_g = torch.cat([film.bias.float() for film in self.films])
                if xd is xs:
                    # ONE [N, 3 R F] projection [H | G] (the kernels read its blocks in place)
                    h = linear(xs, torch.cat([w_h, w_g]), torch.cat([b_g.new_zeros(R * F), b_g]))
                    g = None
                else:
                    h, g = linear(xs, w_h, None), linear(xd, w_g, b_g)
                skip = linear(xd, torch.cat([self.lin_skip.weight.float(),
                                             self.film_skip.weight.float()]), None)
                lin_s, beta_s, gamma_s = skip[:, :F], skip[:, F:2 * F], skip[:, 2 * F:]
            else:  # a caller's module: on the nodes, in the caller's dtype
                h = linear(xs, w_h, None)
                g = torch.cat([film(x_dst).float() for film in self.films], dim=1)
                lin_s = linear(xd, self.lin_skip.weight.float(), None)
                beta_s, gamma_s = self.film_skip(x_dst).float().split(F, dim=-1)
            res = gamma_s * lin_s + beta_s
            if self.act is not None:
                res = self.act(res)
            out = FiLMAggregateFunction.apply(h, g, res[:n_dst], forms, self.act is not None)
        if low is not None and not torch.is_autocast_enabled():
            out = out.to(low)
        return out

    def message(self, x_j: Tensor, beta_i: Tensor, gamma_i: Tensor) -> Tensor:
        out = gamma_i * x_j + beta_i
        if self.act is not None:
            out = self.act(out)
        return out

    def __repr__(self) -> str:
        return (f'{self.__class__.__name__}({self.in_channels}, '
                f'{self.out_channels}, num_relations={self.num_relations})')
