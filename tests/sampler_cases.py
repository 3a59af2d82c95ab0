"""Seeded small leagues that put the samplers on every edge of the forms the host picks from the latent size D,
the covariate count K, the weights and the chain count (tests/test_gpu_sampler_edges.py runs them against
tests/golden/nuts_edge_<case>.npz, which oracle/make_nuts_golden.py writes; tests/test_sampler_cases_host.py
checks on the CPU that every case still sits on the edge it was built for).

The rules are the host's (bpl-next_amd/csrc/bplhip.hip: leaf_in_tail, loop_ok, launch_loop_t,
run_chains_persistent, bplhip_nuts_run) restated in `engines_for`, with every constant read out of the sources, so
that a retuned constant fails the host test instead of silently moving a case off its edge.  What is NOT restated:
that every partition of these leagues is `staged` and that the persistent kernel's grid and LDS fit the device
(loop_ok's other terms) -- the GPU tests assert the engine that actually ran.
"""
import re
from dataclasses import dataclass

import numpy as np

import cases
import dc_oracle as O
from eval_path_cases import _const, _read

_HOST, _NUTS, _KERN = _read("bplhip.hip"), _read("nuts_dev.hip.h"), _read("dc_kernels.hip.h")


def _body(text, head):
    """The text of the function whose signature starts with `head`, up to the first line that closes it."""
    i = text.index(head)
    return text[i:text.index("\n}", i)]


def _one(pattern, text, what):
    found = set(re.findall(pattern, text))
    assert len(found) == 1, (what, found)
    return int(found.pop())


LEAF_NE_MAX = _const(_NUTS, "LEAF_NE_MAX")
KW_NTB = _const(_NUTS, "KW_NTB")
KW_MAX_WG = _const(_NUTS, "KW_MAX_WG")
LOOP_COEF_MAX_K = _const(_KERN, "LOOP_COEF_MAX_K")
XS_STAGED_MAX_K = _one(r"xs_staged = (?:L\.)?K > 0 && (?:L\.)?K <= (\d+);", _KERN, "xs_staged")
GRIDY_MAX_CHAINS = _one(r"int opt_gridy_max_chains = (\d+);", _HOST, "gridy_max_chains")
TAIL_MAX_T = _one(r"c->L\.T <= (\d+)", _body(_HOST, "static bool leaf_in_tail("), "leaf_in_tail T")
TAIL_LANES = _one(r"c->L\.D <= (\d+) \* nd::LEAF_NE_MAX", _body(_HOST, "static bool leaf_in_tail("), "leaf_in_tail D")
LOOP_MAX_D = _one(r"c->L\.D <= (\d+);", _body(_HOST, "bool loop_ok("), "loop_ok D")
LOOP_LNE1_MAX_D = _one(r"if \(c->L\.D > (\d+)\)", _body(_HOST, "int launch_loop_t("), "launch_loop_t D")
TAIL_MAX_D = TAIL_LANES * LEAF_NE_MAX
WAVE = 64

SETTINGS = ("persistent", "kernel0", "device", "host")   # default; persistent_kernel = 0; persistent_nuts = 0; device_nuts = 0
OPTIONS = {"persistent": {}, "kernel0": {"persistent_kernel": 0}, "device": {"persistent_nuts": 0},
           "host": {"device_nuts": 0}}


def kw_workgroups(D):
    return max(1, min(KW_MAX_WG, -(-D // KW_NTB)))


def engines_for(T, D):
    """ENGINE_* name of a single chain under each of SETTINGS (bplhip_nuts_run's dispatch)."""
    tail = T <= TAIL_MAX_T and D <= TAIL_MAX_D
    if tail:
        loop = "LOOP_LNE1" if D <= LOOP_LNE1_MAX_D else "LOOP_LNE2"
        return {"persistent": loop if D <= LOOP_MAX_D else "PERSIST_TAIL", "kernel0": "PERSIST_TAIL",
                "device": "DEVICE_TREE", "host": "HOST_TREE"}
    own = "PERSIST_KP_LEAF" if D <= TAIL_MAX_D else "PERSIST_KW_LEAF"
    return {"persistent": own, "kernel0": own, "device": "HOST_TREE", "host": "HOST_TREE"}


def chains_engine(T, D, n_chains, persistent_nuts=1):
    """ENGINE_* name of bplhip_nuts_run_chains for n_chains > 1."""
    if not (T <= TAIL_MAX_T and D <= TAIL_MAX_D):
        return engines_for(T, D)["persistent"]
    if not persistent_nuts:
        return "LOCKSTEP_VEC"
    return "PERSIST_GRIDY" if n_chains <= GRIDY_MAX_CHAINS else "PERSIST_VEC"


@dataclass(frozen=True)
class Case:
    name: str
    model: int
    T: int
    K: int
    weighted: bool
    D: int
    engines: tuple          # ENGINE_* name per entry of SETTINGS, as DESIGN.md section 40's table states them
    seed: int = 0           # moves the league when the recipe's conditioning check asks for another

    @property
    def n(self):
        return 1500 if self.T <= 64 else 3000

    def engine(self, setting):
        return self.engines[SETTINGS.index(setting)]

    @property
    def bindable(self):
        """bplhip_set_fixtures takes the case: the basic model has neither covariates nor weights."""
        return self.model == O.MODEL_EXTENDED or not (self.weighted or self.K)

    @property
    def tail(self):
        return self.engine("device") == "DEVICE_TREE"


B, E = O.MODEL_BASIC, O.MODEL_EXTENDED
_L1 = ("LOOP_LNE1", "PERSIST_TAIL", "DEVICE_TREE", "HOST_TREE")
_L2 = ("LOOP_LNE2", "PERSIST_TAIL", "DEVICE_TREE", "HOST_TREE")
_TL = ("PERSIST_TAIL", "PERSIST_TAIL", "DEVICE_TREE", "HOST_TREE")
_KP = ("PERSIST_KP_LEAF", "PERSIST_KP_LEAF", "HOST_TREE", "HOST_TREE")
_KW = ("PERSIST_KW_LEAF", "PERSIST_KW_LEAF", "HOST_TREE", "HOST_TREE")
ALL = [
    Case("b63", B, 29, 0, False, 63, _L1),         # LNE 1, lane 63 idle
    Case("e64w", E, 19, 0, True, 64, _L1),         # LNE 1 full wave; weighted + clip loop kernel
    Case("b65", B, 30, 0, False, 65, _L2),         # LNE 2 with one element in slot 1; staged leaf per launch
    Case("b65w", B, 30, 0, True, 65, _L2),         # weighted, no clip
    Case("e77w", E, 20, 5, True, 77, _L2),         # BASELINE config 3's shape, weighted
    Case("e101", E, 20, 17, False, 101, _L2),      # K just past xs_staged
    Case("e127", E, 40, 0, False, 127, _L2),       # LNE 2, last lane idle
    Case("e128w", E, 39, 2, True, 128, _L2, 4),    # LNE 2 full
    Case("e128k32", E, 19, 32, True, 128, _L2, 1), # K = LOOP_COEF_MAX_K
    Case("e127k33", E, 18, 33, False, 127, _L2),   # K past it: coefficients polled one by one
    Case("e129", E, 40, 1, False, 129, _TL),       # loop refused; staged leaf, 3 elements per lane
    Case("e193", E, 60, 3, False, 193, _TL),       # staged leaf, one element in slot 3
    Case("e256", E, 63, 30, False, 256, _TL),      # staged leaf full
    Case("e257", E, 64, 29, False, 257, _KW),      # T <= 64 but the leaf leaves the tail: kw_leaf, one workgroup
    Case("b255", B, 125, 0, False, 255, _KP),      # kp_leaf, last lane idle
    Case("e256g", E, 83, 0, False, 256, _KP),      # kp_leaf full
    Case("b257", B, 126, 0, False, 257, _KW),      # smallest kw_leaf
    Case("b1025", B, 510, 0, False, 1025, _KW),    # second kw_leaf workgroup holds one element
]
CASES = {c.name: c for c in ALL}
ADAPTED = ("e77w", "b65w", "e64w")  # nuts_edge_<case>_adapt_shallow.npz: the weighted loop instantiations (b65w: oracle only)
BITWISE = ("b63", "e64w", "b65", "b65w", "e77w", "e101", "e127", "e128w", "e128k32", "e127k33")
SPEC = ("e128w", "e128k32")
MULTI = ("b65", "e128w", "e193")
MULTI_CHAINS = (2, 8, 9)
PARITY = ("e101", "e128k32", "e127k33")

# every engine value of include/bplhip.h that a league sampler can be dispatched to
LEAGUE_ENGINES = {"HOST_TREE", "DEVICE_TREE", "LOOP_LNE1", "LOOP_LNE2", "PERSIST_TAIL", "PERSIST_GRIDY", "PERSIST_VEC",
                  "PERSIST_KP_LEAF", "PERSIST_KW_LEAF", "LOCKSTEP_VEC"}


def engines_reached():
    """Every engine the GPU tests assert somewhere: the single-chain settings of every case, the chain counts
    of MULTI, and the lock-step run."""
    out = {e for c in ALL for e in c.engines}
    out |= {chains_engine(CASES[n].T, CASES[n].D, k) for n in MULTI for k in MULTI_CHAINS}
    out.add(chains_engine(CASES["e128w"].T, CASES["e128w"].D, 2, persistent_nuts=0))
    return out


_FX = {}


def fixtures(case):
    """The case's league, built as cases.fixtures("wide_N_T") builds its own: h random, a != h, Poisson goals;
    weights float64 formula in float32 storage (cases.float32_weights), raw covariates (the oracle and the
    tests standardise them with O.standardise_covariates)."""
    if isinstance(case, str):
        case = CASES[case]
    if case.name not in _FX:
        n, T = case.n, case.T
        rs = np.random.RandomState(7000 + 1000 * case.seed + case.D + 3 * case.K + int(case.weighted))
        h = rs.randint(0, T, n)
        a = (h + 1 + rs.randint(0, T - 1, n)) % T
        fx = O.Fixtures(h, a, rs.poisson(1.4, n), rs.poisson(1.1, n), T)
        if case.weighted:
            fx.weights = cases.float32_weights(np.linspace(4, 0, n), 1.0)
        if case.K:
            fx.covariates = rs.normal(size=(T, case.K))
        _FX[case.name] = fx
    return _FX[case.name]


def start(case):
    return np.random.RandomState(2).uniform(-0.2, 0.2, case.D)


KEY, STEP, TRANSITIONS = (0, 11), 0.02, 6
# unweighted, many covariates: every transition at STEP diverges at once in the float64 oracle, the chain never leaves
# its start (oracle/make_nuts_golden.py asserts that this list is exactly those cases); a second golden at FINE_STEP
FINE = ("e101", "e127k33", "e256")
FINE_STEP = 0.01
