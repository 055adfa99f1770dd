"""Weights that change in place under a live engine, as tables (test infrastructure, shared by tests/test_weight_lifecycle_cases.py
on the CPU and tests/test_gpu_weight_lifecycle.py on the GPU).

irs_finalize_weights builds a derived arena from the bound weights (influentialrs_amd/csrc/capi.hip: the bf16 catalog and its
norms, the padded bias, the cross-attention constants c_l, the fragment-packed copies of the small / 16-token / wide layer kernels,
the split-precision step streams, the sequence-resident kernel's vector pack, the float16 range statistics), and the header asks
for it "again after any weight changes in place".  Two tables pin that sentence down:

FAMILIES -- every key of synth.irn_state_dict (IRN and evaluator), per-layer keys grouped by kind, each marked live (a change
must move the engine's output) or dead (it must move nothing, not even a byte of the arena).  Dead by the project's own statement
(tests/train_trunk_ref.py, tests/test_gpu_train_trunk.py:_check: the memory of the cross attention is zero): every
multihead_attn.in_proj_weight, and elements [0, 2d) of every multihead_attn.in_proj_bias.

REPRESENTATIVES -- one decode per distinct kernel family of tests/decoder_route_cases.py and of tests/long_window_cases.py (the
Case objects and expected routes of those tables, not restated), the case with the fewest sequences that reaches the family, at
most MAX_SEQS sequences.

Nothing here needs a GPU or the library."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

import decoder_route_cases as RC
import long_window_cases as LW
from influentialrs_amd import synth

SEED_A, SEED_B = 2027, 4099
MAX_SEQS = 2049  # (the 8192 / 8193 pair of the route table adds no kernel family)

# ------------------------------------------------------------------------------------------------------------ tensor families
CROSS_BIAS = "multihead_attn.in_proj_bias"


@dataclass(frozen=True)
class Family:
    id: str
    kind: str                   # the state_dict key, or for a per-layer family the key behind "decoder.layers.<l>."
    per_layer: bool
    live: bool
    reach: str                  # the output a change must move: "rows" (the decoder's) or "scores" (the top-k, and only it)
    part: Optional[str] = None  # None: the whole tensor; "qk" / "v": elements [0, 2d) / [2d, 3d) of a [3d] vector
    evaluator: bool = True      # the key exists in the evaluator's state_dict
    irn: bool = True            # ... and in the IRN's
    also: Tuple[str, ...] = ()  # further outputs a change must move ("r_u": the user factor)

    def layers(self, n_layers: int) -> List[int]:
        """The layers a test changes: the first, a middle and the last one."""
        return sorted({0, n_layers // 2, n_layers - 1}) if self.per_layer else []

    def keys(self, cfg, every_layer: bool = False) -> List[str]:
        """The keys the family changes (every_layer: the keys it stands for)."""
        if not self.per_layer:
            return [self.kind]
        ls = range(cfg.n_layers) if every_layer else self.layers(cfg.n_layers)
        return [f"decoder.layers.{l}.{self.kind}" for l in ls]

    def span(self, cfg, numel: int) -> Tuple[int, int]:
        """The flat element range of a key the family changes."""
        if self.part is None:
            return 0, numel
        assert numel == 3 * cfg.emb_dim
        return (0, 2 * cfg.emb_dim) if self.part == "qk" else (2 * cfg.emb_dim, 3 * cfg.emb_dim)

    def present(self, evaluator: bool) -> bool:
        return self.evaluator if evaluator else self.irn


def _g(key, reach="rows", **kw):
    return Family(key, key, False, True, reach, **kw)


def _l(kind, live=True, part=None):
    return Family(kind + (":" + part if part else ""), kind, True, live, "rows", part)


FAMILIES: List[Family] = [
    _g("item_embedder.weight", evaluator=False),
    _g("word_embedder.weight", irn=False),
    # the user tensors give the factor r_u, an output of the decode, which the IRN mask adds to the attention scores of the
    # allowed keys: both r_u and the rows must move (REFERENCE_UNMOVED names the one window whose rows cannot)
    _g("user_embedder.weight", also=("r_u",), evaluator=False),
    _g("user_mask_layer.weight", also=("r_u",), evaluator=False),
    _g("user_mask_layer.bias", also=("r_u",), evaluator=False),
    _g("pos_embedder.pe"),
    _g("project.weight", reach="scores"),
    _g("project.bias", reach="scores"),
    _l("self_attn.in_proj_weight"), _l("self_attn.in_proj_bias"),
    _l("self_attn.out_proj.weight"), _l("self_attn.out_proj.bias"),
    # the cross attention reads a zero memory: its k = b_k, v = b_v for every key, the softmax is uniform, and what reaches the
    # residual is the constant c_l = W_o b_v + b_o -- W_in and the q / k thirds of b_in reach nothing
    _l("multihead_attn.in_proj_weight", live=False),
    _l(CROSS_BIAS, live=False, part="qk"), _l(CROSS_BIAS, part="v"),
    _l("multihead_attn.out_proj.weight"), _l("multihead_attn.out_proj.bias"),
    _l("linear1.weight"), _l("linear1.bias"), _l("linear2.weight"), _l("linear2.bias"),
    _l("norm1.weight"), _l("norm1.bias"), _l("norm2.weight"), _l("norm2.bias"), _l("norm3.weight"), _l("norm3.bias"),
]
# (representative, family, output) that a change of the family cannot move, by the float64 reference's own result.  c2_nl1_b1
# is ONE window of a ONE-layer model: the consumed row's layer-0 softmax is saturated (scores of +-300), so oracle.decode gives
# the same bits for r_u 0.44 -> 0.93 / 0.009 / 0.53, in float64 and in float32.  It is a property of that window, not of
# one-layer models: c2_nl1_b164's rows do move, as do every other case's.
_ONE_WINDOW = "c2_nl1_b1"
REFERENCE_UNMOVED = {(_ONE_WINDOW, f, "rows") for f in ("user_embedder.weight", "user_mask_layer.weight", "user_mask_layer.bias")}
FAMILY_BY_ID = {f.id: f for f in FAMILIES}
assert len(FAMILY_BY_ID) == len(FAMILIES), "duplicate family ids"


def families(evaluator: bool) -> List[Family]:
    return [f for f in FAMILIES if f.present(evaluator)]


def covered_keys(cfg, evaluator: bool) -> Dict[str, List[Optional[str]]]:
    """key -> the parts of the families that stand for it (a key must come out as [None], or as the two parts of a split)."""
    out: Dict[str, List[Optional[str]]] = {}
    for f in families(evaluator):
        for k in f.keys(cfg, every_layer=True):
            out.setdefault(k, []).append(f.part)
    return out


def state_dicts(cfg, evaluator: bool):
    """(A, B): two state dicts that differ in EVERY tensor.  The positional table does not depend on the seed: B holds it with
    the positions reversed (the same values, so no range statistic moves).  Item row 0 is zero in both."""
    a = synth.irn_state_dict(cfg, SEED_A, evaluator=evaluator)
    b = synth.irn_state_dict(cfg, SEED_B, evaluator=evaluator)
    b["pos_embedder.pe"] = np.ascontiguousarray(a["pos_embedder.pe"][:, ::-1])
    return a, b


def mixed(cfg, a: Dict[str, np.ndarray], b: Dict[str, np.ndarray], fam: Family, keys: Optional[Sequence[str]] = None) -> Dict[str, np.ndarray]:
    """A with the family's elements taken from B, in the family's keys (or in `keys`, some of them)."""
    out = dict(a)
    assert keys is None or set(keys) <= set(fam.keys(cfg))
    for k in (fam.keys(cfg) if keys is None else keys):
        lo, hi = fam.span(cfg, a[k].size)
        t = a[k].copy()
        t.reshape(-1)[lo:hi] = b[k].reshape(-1)[lo:hi]
        out[k] = t
    return out


# ------------------------------------------------------------------------------------------------------------ decode cases
FAMILY_FIELDS = ("embed", "layer", "tail", "seq", "kv_planes", "att_fused", "x6", "npl", "nt")


def kernel_family(c: RC.Case) -> tuple:
    """(embed, layer, tail, seq, kv_planes, att_fused, x6, npl, nt, evaluator, arithmetic, attn) of a case."""
    return tuple(c.route[f] for f in FAMILY_FIELDS) + (c.evaluator, c.gemm, c.attn)


TABLES = {"routes": RC.CASES, "long": LW.CASES}


def _representatives(cases: Sequence[RC.Case]) -> List[RC.Case]:
    best: Dict[tuple, RC.Case] = {}
    for c in cases:  # (table order breaks a tie)
        if c.B <= MAX_SEQS and (kernel_family(c) not in best or c.B < best[kernel_family(c)].B):
            best[kernel_family(c)] = c
    return [c for c in cases if best.get(kernel_family(c)) is c]


@dataclass(frozen=True)
class Rep:
    table: str
    case: RC.Case

    @property
    def id(self):
        return self.case.id

    def group(self):
        """Representatives that share one engine."""
        return (self.table,) + self.case.engine_key()


REPRESENTATIVES: List[Rep] = [Rep(t, c) for t, cases in TABLES.items() for c in _representatives(cases)]
REP_BY_ID = {r.id: r for r in REPRESENTATIVES}
assert len(REP_BY_ID) == len(REPRESENTATIVES), "duplicate representative ids"


def group_seqs(group) -> int:
    return max(r.case.B for r in REPRESENTATIVES if r.group() == group)


def ordered() -> List[Rep]:
    """The representatives grouped by engine, table order otherwise."""
    groups = []
    for r in REPRESENTATIVES:
        if r.group() not in groups:
            groups.append(r.group())
    return sorted(REPRESENTATIVES, key=lambda r: groups.index(r.group()))


def groups() -> List[Rep]:
    """One representative per engine group: the first of ordered()."""
    seen, out = set(), []
    for r in ordered():
        if r.group() not in seen:
            seen.add(r.group())
            out.append(r)
    return out


def _triple(r: Rep):
    return tuple(r.case.route[f] for f in ("embed", "layer", "tail"))


def one_per_kernel_triple() -> List[Rep]:
    """A subset that still holds every (embed, layer, tail) of the representatives once, for the IRN and for the evaluator (its
    state_dict has other keys): the fewest sequences first, and a representative is kept when its triple is new."""
    seen, keep = set(), set()
    for r in sorted(ordered(), key=lambda r: r.case.B):
        key = _triple(r) + (r.case.evaluator,)
        if key not in seen:
            seen.add(key)
            keep.add(r.id)
    return [r for r in ordered() if r.id in keep]


# ------------------------------------------------------------------------------------------------------------ scoring cases
# (n_item, d, rank, world): the direct and the swept top-k with scalar (d = 30) and vector (d = 128) staging; one shard of three,
# which binds a view of the whole tensor
SCORING = [(2085, 30, 0, 1), (4097, 128, 0, 1), (9000, 30, 0, 1), (70_001, 128, 0, 1), (70_001, 128, 1, 3)]
SCORING_ROWS = 33
ARENA_UNWRITTEN_MAX = 2048  # bytes per configuration that finalisation may leave unwritten: six section gaps of < 256 bytes
                            # (derived_plan) and the unused floats of the 256-byte statistics block -- a condition, not a measurement
