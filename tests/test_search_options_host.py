"""not-gpu: which search entry point admits which bound option, through the ABI on contexts created without a device.

Every scenario binds one option (or one of a few pairs) with fake non-null addresses -- binding a trace, a lookahead, a float
guide, the survivor scratch and the arrival rule launches nothing; exclusions need a device and are left to the GPU tests --
then calls every search entry point with otherwise valid arguments and compares the return code and the WHOLE irs_last_error
text against EXPECTED below.  The first failing check of an entry point decides both, so two checks that swap places change a
row.  EXPECTED is a recording of the library as it stood before the option checks were gathered into one rule table
(csrc/capi.hip: search_rules): it was printed by a throwaway script from that build, not written from the code it now guards.

What an admitted call ends at, on a context without weights: the loops at IRS_E_STATE (the readiness check follows the option
rules; the beam loops' trace refusal comes behind it and is therefore never seen here), the two beam steps at their launcher's
own width check (W = 33 passes the entry points and is refused before the launch).  irs_path_step has no check behind its option
rules, so an admitted irs_path_step is a launch: it is called only where a bound guide refuses it."""
import ctypes

import pytest

from influentialrs_amd import _lib

NAN = float("nan")
P = ctypes.c_void_p(4096)  # a fake non-null address: every call here is refused before anything is dereferenced or launched


def _ctx(world=1):
    lib = _lib.load()
    h = ctypes.c_void_p()
    dims = _lib.IrsDims(n_item=1000, n_user=10, d=30, max_len=60, n_heads=6, ffn_dim=256, n_layers=2, u_dim=10, mask_mode=0,
                        max_rows=64, max_k=100, max_seqs=0)
    shard = _lib.IrsShard(0, world, 0, 1000 // world) if world > 1 else None
    assert lib.irs_create(ctypes.byref(h), ctypes.byref(dims), ctypes.byref(shard) if shard else None) == 0
    return lib, h


# ---------------------------------------------------------------- the bindings
def _trace(lib, h):
    return lib.irs_bind_path_trace(h, P, P, P, 8, 4, P, lib.irs_path_trace_scratch_bytes(h, 8))


def _lookahead(lib, h):  # k_c = 3 for 32 users, with a record of 4 steps: 22 users' children are more than max_rows = 64
    return lib.irs_bind_lookahead(h, 3, P, lib.irs_lookahead_scratch_bytes(h, 32, 3), P, P, 32, 4)


def _guide(lib, h):  # a float table of 8 features is read where it lies: no scratch, no launch; k_c = 5
    return lib.irs_bind_guide(h, _lib.IRS_GUIDE_FLOAT, P, 8, 5, None, 0, None)


def _survivors(lib, h):
    return lib.irs_bind_survivor_scratch(h, P, 1 << 20)


def _arrival(lib, h):
    return lib.irs_set_arrival_rule(h, 3, NAN)


BIND = {"trace": _trace, "lookahead": _lookahead, "guide": _guide, "survivors": _survivors, "arrival": _arrival}
SCENARIOS = [(), ("survivors",), ("trace",), ("guide",), ("lookahead",), ("arrival",), ("guide", "lookahead"), ("lookahead", "guide"),
             ("trace", "guide"), ("trace", "lookahead", "arrival")]
SHARDED_SCENARIOS = [(), ("survivors",), ("trace",), ("guide",), ("lookahead",), ("arrival",)]


# ---------------------------------------------------------------- the calls: B = 4 users, path length 3, k = 10 unless named
def _greedy(lib, h, until, k=10, sample=0, B=4, plen=3):
    if until:
        return lib.irs_generate_paths_until(h, P, P, P, B, plen, k, 0, sample, 3, 0, 1, P, P, None, None)
    return lib.irs_generate_paths(h, P, P, P, B, plen, k, 0, sample, 3, 0, 0, P, P, None)


def _calls(lib, h, guide_bound):
    """name -> thunk, in a fixed order.  The variants behind the plain calls walk the greedy side's argument checks (the two
    greedy loops share them: the until loop shows only that it shares their place)."""
    c = {}
    c["irs_generate_paths"] = lambda: _greedy(lib, h, 0)
    c["irs_generate_paths sample=1 k=2"] = lambda: _greedy(lib, h, 0, k=2, sample=1)
    c["irs_generate_paths k=2"] = lambda: _greedy(lib, h, 0, k=2)
    c["irs_generate_paths B=33"] = lambda: _greedy(lib, h, 0, B=33)
    c["irs_generate_paths P=5"] = lambda: _greedy(lib, h, 0, plen=5)
    c["irs_generate_paths B=22"] = lambda: _greedy(lib, h, 0, B=22)
    c["irs_generate_paths_until"] = lambda: _greedy(lib, h, 1)
    c["irs_generate_paths_until sample=1 k=2"] = lambda: _greedy(lib, h, 1, k=2, sample=1)
    if guide_bound:  # (see the module's docstring)
        c["irs_path_step sample=1 k=4"] = lambda: lib.irs_path_step(h, P, P, 4, P, P, 4, 0, P, 3, 1, 3, 0, P, None)
        c["irs_path_step k=4"] = lambda: lib.irs_path_step(h, P, P, 4, P, P, 4, 0, P, 3, 0, 0, 0, P, None)
    c["irs_beam_step"] = lambda: lib.irs_beam_step(h, P, P, P, P, P, P, P, P, 2, 33, 10, 0, 3, P, P, P, P, P, None)
    c["irs_beam_step_until"] = lambda: lib.irs_beam_step_until(h, P, P, P, P, P, P, P, P, P, 2, 33, 10, 0, 3, 0, P, P, P, P, P, P, P, None)
    c["irs_beam_search"] = lambda: lib.irs_beam_search(h, P, P, P, 2, 2, 3, 10, 0, 0, P, P, None, P, None)
    c["irs_beam_search_until"] = lambda: lib.irs_beam_search_until(h, P, P, P, 2, 2, 3, 10, 0, 0, 1, P, P, P, None, P, None, None)
    return c


def _sharded_calls(lib, h, comm):
    return {"irs_generate_paths_sharded": lambda: lib.irs_generate_paths_sharded(h, comm, P, P, P, 4, 3, 100, 0, 0, 0, 0, 0, P, P, None),
            "irs_beam_search_sharded": lambda: lib.irs_beam_search_sharded(h, comm, P, P, P, 2, 2, 3, 100, 0, 0, 0, P, P, None, P, None)}


def _observe(lib, h, bound, calls):
    """[(what, return code, message)]: the binds in order, then every call of calls(guide_bound).  A message is read only
    behind a failure (a successful call leaves the previous text in place)."""
    seen = []
    for name in bound:
        rc = BIND[name](lib, h)
        seen.append(("bind " + name, rc, lib.irs_last_error(h).decode() if rc else ""))
    for what, thunk in calls(("bind guide", 0, "") in seen).items():
        rc = thunk()
        seen.append((what, rc, lib.irs_last_error(h).decode() if rc else ""))
    return seen


def observe_single(bound):
    lib, h = _ctx()
    try:
        return _observe(lib, h, bound, lambda guide_bound: _calls(lib, h, guide_bound))
    finally:
        lib.irs_destroy(h)


def observe_sharded(bound):
    lib, h = _ctx(world=2)
    comm = ctypes.c_void_p()

    def never(*a):  # pragma: no cover
        raise AssertionError("a collective ran")

    cbs = (_lib.ALLGATHER_FN(never), _lib.ALLTOALL_FN(never), _lib.ALLREDUCE_F32_FN(never))
    assert lib.irs_comm_init_callbacks(ctypes.byref(comm), 0, 2, None, *(ctypes.cast(cb, ctypes.c_void_p) for cb in cbs)) == 0
    try:
        return _observe(lib, h, bound, lambda guide_bound: _sharded_calls(lib, h, comm))
    finally:
        lib.irs_comm_destroy(comm)
        lib.irs_destroy(h)


# recorded from the parent of the commit that added this file (see the module's docstring)
EXPECTED = {
    (): [
        ('irs_generate_paths', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_generate_paths sample=1 k=2', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_generate_paths k=2', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_generate_paths B=33', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_generate_paths P=5', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_generate_paths B=22', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_generate_paths_until', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_generate_paths_until sample=1 k=2', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_beam_step', -4, 'beam width 33 outside [1, 32]'),
        ('irs_beam_step_until', -4, 'beam width 33 outside [1, 32]'),
        ('irs_beam_search', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_beam_search_until', -2, 'weights not finalized (irs_finalize_weights)'),
    ],
    ('survivors',): [
        ('bind survivors', 0, ''),
        ('irs_generate_paths', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_generate_paths sample=1 k=2', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_generate_paths k=2', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_generate_paths B=33', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_generate_paths P=5', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_generate_paths B=22', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_generate_paths_until', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_generate_paths_until sample=1 k=2', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_beam_step', -4, 'beam width 33 outside [1, 32]'),
        ('irs_beam_step_until', -4, 'beam width 33 outside [1, 32]'),
        ('irs_beam_search', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_beam_search_until', -2, 'weights not finalized (irs_finalize_weights)'),
    ],
    ('trace',): [
        ('bind trace', 0, ''),
        ('irs_generate_paths', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_generate_paths sample=1 k=2', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_generate_paths k=2', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_generate_paths B=33', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_generate_paths P=5', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_generate_paths B=22', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_generate_paths_until', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_generate_paths_until sample=1 k=2', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_beam_step', -4, 'irs_beam_step: a path trace is bound (irs_bind_path_trace): greedy and sampled loops only'),
        ('irs_beam_step_until', -4, 'irs_beam_step_until: a path trace is bound (irs_bind_path_trace): greedy and sampled loops only'),
        ('irs_beam_search', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_beam_search_until', -2, 'weights not finalized (irs_finalize_weights)'),
    ],
    ('guide',): [
        ('bind guide', 0, ''),
        ('irs_generate_paths', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_generate_paths sample=1 k=2', -4,
         'irs_generate_paths: a guide is bound (irs_bind_guide): the guided choice is deterministic, sample must be 0'),
        ('irs_generate_paths k=2', -1, 'irs_generate_paths: a guide is bound (irs_bind_guide): k=2 < k_c=5'),
        ('irs_generate_paths B=33', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_generate_paths P=5', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_generate_paths B=22', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_generate_paths_until', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_generate_paths_until sample=1 k=2', -4,
         'irs_generate_paths_until: a guide is bound (irs_bind_guide): the guided choice is deterministic, sample must be 0'),
        ('irs_path_step sample=1 k=4', -4, 'irs_path_step: a guide is bound (irs_bind_guide): the guided choice is deterministic, sample must be 0'),
        ('irs_path_step k=4', -1, 'irs_path_step: a guide is bound (irs_bind_guide): k=4 < k_c=5'),
        ('irs_beam_step', -4, 'irs_beam_step: a guide is bound (irs_bind_guide): greedy loops only'),
        ('irs_beam_step_until', -4, 'irs_beam_step_until: a guide is bound (irs_bind_guide): greedy loops only'),
        ('irs_beam_search', -4, 'irs_beam_search: a guide is bound (irs_bind_guide): greedy loops only'),
        ('irs_beam_search_until', -4, 'irs_beam_search_until: a guide is bound (irs_bind_guide): greedy loops only'),
    ],
    ('lookahead',): [
        ('bind lookahead', 0, ''),
        ('irs_generate_paths', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_generate_paths sample=1 k=2', -4,
         'irs_generate_paths: a lookahead is bound (irs_bind_lookahead): the choice is deterministic, sample must be 0'),
        ('irs_generate_paths k=2', -1, 'irs_generate_paths: a lookahead is bound (irs_bind_lookahead): k=2 < k_c=3'),
        ('irs_generate_paths B=33', -1, 'irs_generate_paths: B=33, the lookahead is bound for 32 users'),
        ('irs_generate_paths P=5', -1, 'irs_generate_paths: path length 5, the lookahead record is bound for 4 steps'),
        ('irs_generate_paths B=22', -1, 'irs_generate_paths: a lookahead is bound (irs_bind_lookahead): B*k_c=66 exceeds max_seqs=64 / max_rows=64'),
        ('irs_generate_paths_until', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_generate_paths_until sample=1 k=2', -4,
         'irs_generate_paths_until: a lookahead is bound (irs_bind_lookahead): the choice is deterministic, sample must be 0'),
        ('irs_beam_step', -4, 'irs_beam_step: a lookahead is bound (irs_bind_lookahead): greedy loops only'),
        ('irs_beam_step_until', -4, 'irs_beam_step_until: a lookahead is bound (irs_bind_lookahead): greedy loops only'),
        ('irs_beam_search', -4, 'irs_beam_search: a lookahead is bound (irs_bind_lookahead): greedy loops only'),
        ('irs_beam_search_until', -4, 'irs_beam_search_until: a lookahead is bound (irs_bind_lookahead): greedy loops only'),
    ],
    ('arrival',): [
        ('bind arrival', 0, ''),
        ('irs_generate_paths', -2,
         'irs_generate_paths: an arrival rule is set (irs_set_arrival_rule) and no path trace is bound (irs_bind_path_trace): the rule reads what the trace records'),
        ('irs_generate_paths sample=1 k=2', -2,
         'irs_generate_paths: an arrival rule is set (irs_set_arrival_rule) and no path trace is bound (irs_bind_path_trace): the rule reads what the trace records'),
        ('irs_generate_paths k=2', -2,
         'irs_generate_paths: an arrival rule is set (irs_set_arrival_rule) and no path trace is bound (irs_bind_path_trace): the rule reads what the trace records'),
        ('irs_generate_paths B=33', -2,
         'irs_generate_paths: an arrival rule is set (irs_set_arrival_rule) and no path trace is bound (irs_bind_path_trace): the rule reads what the trace records'),
        ('irs_generate_paths P=5', -2,
         'irs_generate_paths: an arrival rule is set (irs_set_arrival_rule) and no path trace is bound (irs_bind_path_trace): the rule reads what the trace records'),
        ('irs_generate_paths B=22', -2,
         'irs_generate_paths: an arrival rule is set (irs_set_arrival_rule) and no path trace is bound (irs_bind_path_trace): the rule reads what the trace records'),
        ('irs_generate_paths_until', -2,
         'irs_generate_paths_until: an arrival rule is set (irs_set_arrival_rule) and no path trace is bound (irs_bind_path_trace): the rule reads what the trace records'),
        ('irs_generate_paths_until sample=1 k=2', -2,
         'irs_generate_paths_until: an arrival rule is set (irs_set_arrival_rule) and no path trace is bound (irs_bind_path_trace): the rule reads what the trace records'),
        ('irs_beam_step', -4, 'beam width 33 outside [1, 32]'),
        ('irs_beam_step_until', -4, 'beam width 33 outside [1, 32]'),
        ('irs_beam_search', -4, 'irs_beam_search: an arrival rule is set (irs_set_arrival_rule): greedy and sampled loops only'),
        ('irs_beam_search_until', -4, 'irs_beam_search_until: an arrival rule is set (irs_set_arrival_rule): greedy and sampled loops only'),
    ],
    ('guide', 'lookahead'): [
        ('bind guide', 0, ''),
        ('bind lookahead', -4, 'irs_bind_lookahead: a guide is bound (irs_bind_guide): one choice rule at a time'),
        ('irs_generate_paths', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_generate_paths sample=1 k=2', -4,
         'irs_generate_paths: a guide is bound (irs_bind_guide): the guided choice is deterministic, sample must be 0'),
        ('irs_generate_paths k=2', -1, 'irs_generate_paths: a guide is bound (irs_bind_guide): k=2 < k_c=5'),
        ('irs_generate_paths B=33', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_generate_paths P=5', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_generate_paths B=22', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_generate_paths_until', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_generate_paths_until sample=1 k=2', -4,
         'irs_generate_paths_until: a guide is bound (irs_bind_guide): the guided choice is deterministic, sample must be 0'),
        ('irs_path_step sample=1 k=4', -4, 'irs_path_step: a guide is bound (irs_bind_guide): the guided choice is deterministic, sample must be 0'),
        ('irs_path_step k=4', -1, 'irs_path_step: a guide is bound (irs_bind_guide): k=4 < k_c=5'),
        ('irs_beam_step', -4, 'irs_beam_step: a guide is bound (irs_bind_guide): greedy loops only'),
        ('irs_beam_step_until', -4, 'irs_beam_step_until: a guide is bound (irs_bind_guide): greedy loops only'),
        ('irs_beam_search', -4, 'irs_beam_search: a guide is bound (irs_bind_guide): greedy loops only'),
        ('irs_beam_search_until', -4, 'irs_beam_search_until: a guide is bound (irs_bind_guide): greedy loops only'),
    ],
    ('lookahead', 'guide'): [
        ('bind lookahead', 0, ''),
        ('bind guide', -4, 'irs_bind_guide: a lookahead is bound (irs_bind_lookahead): one choice rule at a time'),
        ('irs_generate_paths', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_generate_paths sample=1 k=2', -4,
         'irs_generate_paths: a lookahead is bound (irs_bind_lookahead): the choice is deterministic, sample must be 0'),
        ('irs_generate_paths k=2', -1, 'irs_generate_paths: a lookahead is bound (irs_bind_lookahead): k=2 < k_c=3'),
        ('irs_generate_paths B=33', -1, 'irs_generate_paths: B=33, the lookahead is bound for 32 users'),
        ('irs_generate_paths P=5', -1, 'irs_generate_paths: path length 5, the lookahead record is bound for 4 steps'),
        ('irs_generate_paths B=22', -1, 'irs_generate_paths: a lookahead is bound (irs_bind_lookahead): B*k_c=66 exceeds max_seqs=64 / max_rows=64'),
        ('irs_generate_paths_until', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_generate_paths_until sample=1 k=2', -4,
         'irs_generate_paths_until: a lookahead is bound (irs_bind_lookahead): the choice is deterministic, sample must be 0'),
        ('irs_beam_step', -4, 'irs_beam_step: a lookahead is bound (irs_bind_lookahead): greedy loops only'),
        ('irs_beam_step_until', -4, 'irs_beam_step_until: a lookahead is bound (irs_bind_lookahead): greedy loops only'),
        ('irs_beam_search', -4, 'irs_beam_search: a lookahead is bound (irs_bind_lookahead): greedy loops only'),
        ('irs_beam_search_until', -4, 'irs_beam_search_until: a lookahead is bound (irs_bind_lookahead): greedy loops only'),
    ],
    ('trace', 'guide'): [
        ('bind trace', 0, ''),
        ('bind guide', 0, ''),
        ('irs_generate_paths', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_generate_paths sample=1 k=2', -4,
         'irs_generate_paths: a guide is bound (irs_bind_guide): the guided choice is deterministic, sample must be 0'),
        ('irs_generate_paths k=2', -1, 'irs_generate_paths: a guide is bound (irs_bind_guide): k=2 < k_c=5'),
        ('irs_generate_paths B=33', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_generate_paths P=5', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_generate_paths B=22', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_generate_paths_until', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_generate_paths_until sample=1 k=2', -4,
         'irs_generate_paths_until: a guide is bound (irs_bind_guide): the guided choice is deterministic, sample must be 0'),
        ('irs_path_step sample=1 k=4', -4, 'irs_path_step: a guide is bound (irs_bind_guide): the guided choice is deterministic, sample must be 0'),
        ('irs_path_step k=4', -1, 'irs_path_step: a guide is bound (irs_bind_guide): k=4 < k_c=5'),
        ('irs_beam_step', -4, 'irs_beam_step: a path trace is bound (irs_bind_path_trace): greedy and sampled loops only'),
        ('irs_beam_step_until', -4, 'irs_beam_step_until: a path trace is bound (irs_bind_path_trace): greedy and sampled loops only'),
        ('irs_beam_search', -4, 'irs_beam_search: a guide is bound (irs_bind_guide): greedy loops only'),
        ('irs_beam_search_until', -4, 'irs_beam_search_until: a guide is bound (irs_bind_guide): greedy loops only'),
    ],
    ('trace', 'lookahead', 'arrival'): [
        ('bind trace', 0, ''),
        ('bind lookahead', 0, ''),
        ('bind arrival', 0, ''),
        ('irs_generate_paths', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_generate_paths sample=1 k=2', -4,
         'irs_generate_paths: a lookahead is bound (irs_bind_lookahead): the choice is deterministic, sample must be 0'),
        ('irs_generate_paths k=2', -1, 'irs_generate_paths: a lookahead is bound (irs_bind_lookahead): k=2 < k_c=3'),
        ('irs_generate_paths B=33', -1, 'irs_generate_paths: B=33, the lookahead is bound for 32 users'),
        ('irs_generate_paths P=5', -1, 'irs_generate_paths: path length 5, the lookahead record is bound for 4 steps'),
        ('irs_generate_paths B=22', -1, 'irs_generate_paths: a lookahead is bound (irs_bind_lookahead): B*k_c=66 exceeds max_seqs=64 / max_rows=64'),
        ('irs_generate_paths_until', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_generate_paths_until sample=1 k=2', -4,
         'irs_generate_paths_until: a lookahead is bound (irs_bind_lookahead): the choice is deterministic, sample must be 0'),
        ('irs_beam_step', -4, 'irs_beam_step: a path trace is bound (irs_bind_path_trace): greedy and sampled loops only'),
        ('irs_beam_step_until', -4, 'irs_beam_step_until: a path trace is bound (irs_bind_path_trace): greedy and sampled loops only'),
        ('irs_beam_search', -4, 'irs_beam_search: a lookahead is bound (irs_bind_lookahead): greedy loops only'),
        ('irs_beam_search_until', -4, 'irs_beam_search_until: a lookahead is bound (irs_bind_lookahead): greedy loops only'),
    ],
}
EXPECTED_SHARDED = {
    (): [
        ('irs_generate_paths_sharded', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_beam_search_sharded', -2, 'weights not finalized (irs_finalize_weights)'),
    ],
    ('survivors',): [
        ('bind survivors', 0, ''),
        ('irs_generate_paths_sharded', -4,
         'irs_generate_paths_sharded: exact candidates (irs_bind_survivor_scratch) need the whole catalog on one device'),
        ('irs_beam_search_sharded', -4, 'irs_beam_search_sharded: exact candidates (irs_bind_survivor_scratch) need the whole catalog on one device'),
    ],
    ('trace',): [
        ('bind trace', -4, 'irs_bind_path_trace needs the whole catalog on one device'),
        ('irs_generate_paths_sharded', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_beam_search_sharded', -2, 'weights not finalized (irs_finalize_weights)'),
    ],
    ('guide',): [
        ('bind guide', -4, 'irs_bind_guide needs the whole catalog on one device'),
        ('irs_generate_paths_sharded', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_beam_search_sharded', -2, 'weights not finalized (irs_finalize_weights)'),
    ],
    ('lookahead',): [
        ('bind lookahead', -4, 'irs_bind_lookahead needs the whole catalog on one device'),
        ('irs_generate_paths_sharded', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_beam_search_sharded', -2, 'weights not finalized (irs_finalize_weights)'),
    ],
    ('arrival',): [
        ('bind arrival', -4, 'irs_set_arrival_rule needs the whole catalog on one device'),
        ('irs_generate_paths_sharded', -2, 'weights not finalized (irs_finalize_weights)'),
        ('irs_beam_search_sharded', -2, 'weights not finalized (irs_finalize_weights)'),
    ],
}


@pytest.mark.parametrize("bound", SCENARIOS, ids=lambda b: "+".join(b) or "nothing")
def test_every_entry_point_answers_a_bound_option_as_recorded(bound):
    seen = observe_single(bound)
    want = EXPECTED[bound]
    assert [s[0] for s in seen] == [w[0] for w in want], "the recording covers other calls: record it again from the parent"
    for got, exp in zip(seen, want):
        assert got == exp


@pytest.mark.parametrize("bound", SHARDED_SCENARIOS, ids=lambda b: "+".join(b) or "nothing")
def test_the_sharded_loops_answer_a_bound_option_as_recorded(bound):
    seen = observe_sharded(bound)
    assert seen == EXPECTED_SHARDED[bound]


def test_the_recording_distinguishes_the_order_of_checks():
    """The table is a net for swapped checks only if neighbouring checks give different answers: say so for the orders the
    entry points keep on purpose."""
    row = {b: {w: (rc, msg) for w, rc, msg in rows} for b, rows in EXPECTED.items()}
    # arrival without a trace is looked at before a bound lookahead's arguments, and both before the readiness check
    both = row[("trace", "lookahead", "arrival")]
    assert row[("arrival",)]["irs_generate_paths"][0] == -2 and "no path trace is bound" in row[("arrival",)]["irs_generate_paths"][1]
    assert "sample must be 0" in both["irs_generate_paths sample=1 k=2"][1] and "k=2 < k_c=3" in both["irs_generate_paths k=2"][1]
    assert "for 32 users" in both["irs_generate_paths B=33"][1] and "B*k_c=66" in both["irs_generate_paths B=22"][1]
    assert "weights not finalized" in both["irs_generate_paths"][1]
    # the beam loops: guide, then lookahead, then the arrival rule, then readiness; the trace only behind it
    assert "irs_bind_lookahead" in both["irs_beam_search"][1] and "irs_set_arrival_rule" in row[("arrival",)]["irs_beam_search"][1]
    assert "weights not finalized" in row[("trace",)]["irs_beam_search"][1]
    # the beam steps: trace, then guide, then lookahead; neither the arrival rule nor the scratch
    assert "irs_bind_path_trace" in row[("trace", "guide")]["irs_beam_step"][1] and "irs_bind_path_trace" in both["irs_beam_step_until"][1]
    assert "beam width 33" in row[("arrival",)]["irs_beam_step"][1] and "beam width 33" in row[("survivors",)]["irs_beam_step_until"][1]
