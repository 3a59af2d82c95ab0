#!/usr/bin/env python3
"""Parent tree against working tree, byte for byte: every model class fitted and queried through the
public API by both copies of bpl-next_amd/bpl, in one child process per tree, against the working
tree's libbplhip.so (BPLHIP_LIB).

  python tools/fit_ab.py --parent REV --stub    # CPU: recording stub context (tests/fake_ctx.py)
  python tools/fit_ab.py --parent REV           # GPU: the real context, short chains
  python tools/fit_ab.py --parent-dir DIR       # the parent's package already unpacked (DIR/bpl)
  ... --self                                    # additionally the parent against itself, first

One of --parent and --parent-dir is required: REV is the commit to compare the working tree against
(`git archive REV bpl-next_amd/bpl`, unpacked into a temporary directory).  In --stub mode the context logs every call the fit makes on it (which
set_fixtures*, with which arrays; the NUTS configuration; keys and start points per nuts_run /
nuts_run_chains; constrain*; close) and the logs are compared too; predict calls go to
tests/fake_ctx.py:FakePredictCtx, and a method it lacks ends that case after the host checks (the
AttributeError is the recorded result on both sides).  Compared: call logs, every public attribute of
every fitted model, mcmc_info_ without wall_seconds, every predict result (differing bytes per array),
exception type and message of every failing case.  Only the failures the cases are written to provoke
are recorded (host-side argument errors, and a library error with an argument code); anything else, a
device fault above all, ends the child there, and with it the whole run.  Exit status 3 on any difference that is not among
the ACCEPTED_* ones below."""
import argparse
import os
import pickle
import subprocess
import sys
import tempfile
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the only differences the shared fit driver may show against its parent, each reported line by line
ACCEPTED_NEW_KEYS = "mcmc_info_ gains the keys the league classes already have"
ACCEPTED_EARLIER = "the check runs before a context is created (the parent created, bound and closed one first)"
# what a case may raise and have recorded as its result (include/bplhip.h: -1 EINVAL, -5 EUNSUPPORTED)
HOST_ERRORS = (ValueError, TypeError, KeyError, IndexError, NotImplementedError, AttributeError)
ARGUMENT_CODES = (-1, -5)
ACCEPTED_MESSAGES = {
    "num_chains and thinning must be positive": "num_chains and thinning must be >= 1",
}


# ----------------------------------------------------------------------------- the cases (child side)
def _data(seed=0, T=6, n=40):
    rs = np.random.RandomState(seed)
    h = rs.randint(0, T, n)
    a = (h + 1 + rs.randint(0, T - 1, n)) % T
    names = np.array([str(i) for i in range(T)])
    d = {"home_team": names[h], "away_team": names[a], "home_goals": rs.poisson(1.4, n), "away_goals": rs.poisson(1.1, n),
         "time_diff": rs.uniform(0, 3, n), "game_weights": rs.uniform(0.5, 2.0, n), "neutral_venue": rs.randint(0, 2, n),
         "gameweek": np.sort(rs.randint(0, 3, n)), "team_covariates": {t: rs.normal(size=2) for t in names}}
    d["gameweek"][-1] = 2
    conf = np.array(["A", "B", "C"])[np.arange(T) % 3]
    d["home_conf"], d["away_conf"] = conf[h], conf[a]
    return d


def _only(d, *drop):
    return {k: v for k, v in d.items() if k not in drop}


def _fits():
    """(case name, class name, fit kwargs, data)."""
    from bpl._mcmc import latent_sites as league_sites
    from bpl._ffi import MODEL_EXTENDED

    d = _data()
    plain = _only(d, "team_covariates")
    T, K = 6, 2
    rs = np.random.RandomState(7)
    ext_dict = {nm: 0.1 * rs.standard_normal(sz) for nm, sz in league_sites(MODEL_EXTENDED, T, K)}
    D_ext, D_neu, D_dyn = 3 * T + 2 * K + 7, 6 * T + 13, 7 * 3 * T + 10 * 3 + 2
    run = {"num_warmup": 30, "num_samples": 30}
    chains = lambda n, **kw: {"mcmc_kwargs": dict(num_chains=n, **kw), **run}
    fits = [
        ("basic_1", "Basic", run, plain),
        ("basic_3_parallel", "Basic", chains(3, chain_method="parallel"), plain),
        ("basic_3_sequential", "Basic", chains(3, chain_method="sequential"), plain),
        ("basic_thin_extra", "Basic", {**chains(2, thinning=3), "run_kwargs": {"extra_fields": ("num_steps", "accept_prob")}}, plain),
        ("ext_cov_dict", "Extended", {**chains(2), "epsilon": 0.3, "rescale_weights": True, "run_kwargs": {"init_params": ext_dict}}, d),
        ("ext_init_array", "Extended", {**chains(2), "run_kwargs": {"init_params": 0.05 * rs.standard_normal(2 * D_ext)}}, d),
        ("ext_init_one_point", "Extended", {**chains(2), "run_kwargs": {"init_params": 0.05 * rs.standard_normal(D_ext)}}, d),
        ("neutral_1", "Neutral", {**run, "epsilon": 0.2}, plain),
        ("neutral_3_init", "Neutral", {**chains(3), "run_kwargs": {"init_params": 0.05 * rs.standard_normal(D_neu)}}, plain),
        ("neutral_cov_seq", "Neutral", chains(2, chain_method="sequential"), d),
        ("wc_2", "WC", {**chains(2), "epsilon": 0.1, "rescale_weights": True}, plain),
        ("dynamic_walk_cov", "Dynamic", {**chains(2), "random_walk": True}, d),
        ("dynamic_nowalk", "Dynamic", {**chains(2), "random_walk": False}, plain),
        ("dynamic_init", "Dynamic", {**run, "random_walk": False, "run_kwargs": {"init_params": 0.05 * rs.standard_normal(D_dyn)}}, plain),
        # argument rules (each fit raises, or ignores what it ignores today)
        ("basic_bad_key", "Basic", {"mcmc_kwargs": {"nonsense": 1}}, plain),
        ("basic_bad_run_key", "Basic", {"run_kwargs": {"nonsense": 1}}, plain),
        ("basic_bad_chains", "Basic", {"mcmc_kwargs": {"num_chains": 0}}, plain),
        ("basic_bad_method", "Basic", {"mcmc_kwargs": {"chain_method": "bogus"}}, plain),
        ("basic_postprocess", "Basic", {"mcmc_kwargs": {"postprocess_fn": abs}}, plain),
        ("basic_extra_energy", "Basic", {"run_kwargs": {"extra_fields": ("energy",)}}, plain),
        ("basic_bad_goals", "Basic", {}, {**plain, "home_goals": plain["home_goals"] - 1}),
        ("ext_init_missing_site", "Extended", {**run, "run_kwargs": {"init_params": _only(ext_dict, "u")}}, d),
        ("ext_init_bad_size", "Extended", {**chains(2), "run_kwargs": {"init_params": np.zeros(D_ext + 1)}}, d),
        ("ext_cov_missing_team", "Extended", run, {**d, "team_covariates": _only(d["team_covariates"], "3")}),
        ("ext_no_time_diff", "Extended", {**run, "epsilon": 0.1}, _only(d, "time_diff")),
        ("neutral_bad_key", "Neutral", {"mcmc_kwargs": {"nonsense": 1}}, plain),
        ("neutral_bad_chains", "Neutral", {"mcmc_kwargs": {"thinning": 0}}, plain),
        ("neutral_bad_method", "Neutral", {"mcmc_kwargs": {"chain_method": "bogus"}}, plain),
        ("neutral_ignores_postprocess_extra", "Neutral", {**run, "mcmc_kwargs": {"postprocess_fn": abs}, "run_kwargs": {"extra_fields": ("energy",)}}, plain),
        ("neutral_init_bad_size", "Neutral", {**chains(2), "run_kwargs": {"init_params": np.zeros(D_neu + 1)}}, plain),
        ("wc_bad_method", "WC", {"mcmc_kwargs": {"chain_method": "bogus"}}, plain),
        ("dynamic_ignores_keywords", "Dynamic", {**run, "random_walk": False, "mcmc_kwargs": {"chain_method": "bogus", "nonsense": 1}, "run_kwargs": {"nonsense": 2}}, plain),
        ("dynamic_bad_gameweek", "Dynamic", run, {**plain, "gameweek": plain["gameweek"] - 1}),
    ]
    return fits


def _classes():
    from bpl import (DixonColesMatchPredictor, ExtendedDixonColesMatchPredictor, NeutralDixonColesMatchPredictor,
                     NeutralDixonColesMatchPredictorWC)
    from bpl.dynamic_dixon_coles import DynamicNeutralDixonColesMatchPredictor

    return {"Basic": DixonColesMatchPredictor, "Extended": ExtendedDixonColesMatchPredictor,
            "Neutral": NeutralDixonColesMatchPredictor, "WC": NeutralDixonColesMatchPredictorWC,
            "Dynamic": DynamicNeutralDixonColesMatchPredictor}


def _predict_calls(kind, d):
    """(name, method, args, kwargs) for a fitted model of this kind: every predict-side method with a
    fixed random_state, and the argument checks of the simulation methods."""
    H, A, nv = ["0", "1", "2"], ["3", "4", "5"], [0, 1, 0]
    conf = (["A", "B", "C"], ["A", "B", "C"])
    fixtures = {"Basic": (H, A), "Extended": (H, A), "Neutral": (H, A, nv), "WC": (H, A, *conf, nv), "Dynamic": (H, A, nv)}[kind]
    pair = {"WC": ("0", "1", "A", "B")}.get(kind, ("0", "1"))
    calls = [("expected_goals", "_calculate_expected_goals", fixtures, {})]
    if kind == "Dynamic":
        calls += [("score_proba", "predict_score_proba", (H, A, [1, 0, 2], [0, 0, 1], nv), {}),
                  ("score_proba_week0", "predict_score_proba", (H, A, 1, 1, nv), {"gameweek": 0}),
                  ("outcome", "predict_outcome_proba", fixtures, {}),
                  ("outcome_week1", "predict_outcome_proba", fixtures, {"gameweek": 1}),
                  ("outcome_bad_week", "predict_outcome_proba", fixtures, {"gameweek": 9})]
    else:
        goals = ([1, 0, 2], [0, 0, 1])
        score_args = {"Neutral": (H, A, *goals, nv), "WC": (H, A, *conf, *goals, nv)}.get(kind, (H, A, *goals))
        ko = [{}] if kind in ("Basic", "Extended") else [{}, {"knockout": True}]
        calls += [("score_proba", "predict_score_proba", score_args, {}),
                  ("grid", "predict_score_grid_proba", fixtures, {"max_goals": 4}),
                  ("grid_deep", "predict_score_grid_proba", tuple(f[:1] for f in fixtures), {"max_goals": 64}),
                  ("grid_bad_depth", "predict_score_grid_proba", fixtures, {"max_goals": -1}),
                  ("sample_score", "sample_score", fixtures, {"num_samples": 7, "random_state": 11}),
                  ("sample_score_shallow", "sample_score", fixtures, {"num_samples": 3, "random_state": 5, "max_goals": 3})]
        for k in ko:
            tag = "_ko" if k else ""
            calls += [("outcome" + tag, "predict_outcome_proba", fixtures, dict(k)),
                      ("sample_outcome" + tag, "sample_outcome", fixtures, {"num_samples": 9, "random_state": 13, **k})]
        for home in (True, False):
            for meth in ("predict_score_n_proba", "predict_concede_n_proba"):
                calls += [(f"{meth}_{home}", meth, (np.arange(6), *pair), {"home": home}),
                          (f"{meth}_{home}_deep", meth, (18, *pair), {"home": home, "max_goals": 5})]
        calls += [("n_proba_negative", "predict_score_n_proba", (-1, *pair), {}),
                  ("unknown_team", "predict_outcome_proba", (["nobody"],) + tuple(fixtures[1:]), {})]
        if kind != "Basic" and kind != "Extended":
            calls += [("n_proba_neutral", "predict_score_n_proba", (np.arange(4), *pair), {"neutral_venue": 1})]
    season = {"home_team": H, "away_team": A}
    if kind in ("Basic", "Extended"):
        ok = {"num_simulations": 50, "random_state": 3, "current_table": {"0": (3, 2, 1)}}
        calls += [("season", "simulate_season", (H, A), ok),
                  ("season_float_table", "simulate_season", (H, A), {**ok, "current_table": {"0": (3.0, 2, 1)}}),
                  ("season_bad_points", "simulate_season", (H, A), {**ok, "points": (3, 1)}),
                  ("season_bool_points", "simulate_season", (H, A), {**ok, "points": (True, 1, 0)}),
                  ("season_big_points", "simulate_season", (H, A), {**ok, "points": (1001, 1, 0)}),
                  ("season_bad_sims", "simulate_season", (H, A), {**ok, "num_simulations": 0}),
                  ("season_float_sims", "simulate_season", (H, A), {**ok, "num_simulations": 10.0}),
                  ("season_self_play", "simulate_season", (H, H), ok)]
    if kind in ("Neutral", "WC"):
        tc = {"team_conf": {str(i): "ABC"[i % 3] for i in range(6)}} if kind == "WC" else {}
        groups = {"g": ["0", "1", "2"], "h": ["3", "4", "5"]}
        ko4 = [("g", 1), ("h", 2), ("h", 1), ("g", 2)]
        ok = {"groups": groups, "num_simulations": 40, "random_state": 3, **tc}
        calls += [("tournament", "simulate_tournament", (ko4,), ok),
                  ("tournament_knockout_only", "simulate_tournament", (["0", "1", "2", "3"],), {"num_simulations": 40, "random_state": 4, **tc}),
                  ("tournament_float_table", "simulate_tournament", (ko4,), {**ok, "current_table": {"0": (3.0, 2, 1)}}),
                  ("tournament_bad_points", "simulate_tournament", (ko4,), {**ok, "points": "abc"}),
                  ("tournament_big_points", "simulate_tournament", (ko4,), {**ok, "points": (3, 1, 1001)}),
                  ("tournament_bad_sims", "simulate_tournament", (ko4,), {**ok, "num_simulations": True}),
                  ("tournament_huge_sims", "simulate_tournament", (ko4,), {**ok, "num_simulations": 2 ** 31}),
                  ("tournament_bad_bracket", "simulate_tournament", (ko4[:3],), ok)]
    data = {**season, "home_goals": [1, 0, 2], "away_goals": [0, 0, 1], "neutral_venue": nv, "gameweek": [0, 1, 2],
            "home_conf": conf[0], "away_conf": conf[1]}
    calls += [("ppc", "posterior_predictive_check", (data,), {"num_replications": 20, "random_state": 9}),
              ("ppc_bad_points", "posterior_predictive_check", (data,), {"points": (3, 1, -1)}),
              ("ppc_bad_replications", "posterior_predictive_check", (data,), {"num_replications": 0}),
              ("ppc_bad_goals", "posterior_predictive_check", (data,), {"max_goals": 16}),
              ("log_likelihood", "log_likelihood", (data,), {})]
    return calls


def _attempt(fn):
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return fn()
    except HOST_ERRORS as e:
        return ("EXC", type(e).__name__, str(e))
    except Exception as e:  # pylint: disable=broad-except
        # a libbplhip error counts as a result only with an argument code; a device fault, a time-out or
        # anything unforeseen propagates: the child exits non-zero and nothing more is started on the GPU
        if type(e).__name__ == "BplHipError" and getattr(e, "code", None) in ARGUMENT_CODES:
            return ("EXC", type(e).__name__, str(e))
        raise


def child(stub, dump):
    """Run every case on the `bpl` this process imports; pickle {case: {path: value}} to `dump`."""
    import bpl._ffi as ffi

    ctx_cls = None
    if stub:
        from fake_ctx import FakePredictCtx, RecordingCtx

        ffi.HipContext = ctx_cls = RecordingCtx
    out = {}
    for name, kind, kwargs, data in _fits():
        if stub:
            ctx_cls.reset()
        model = _classes()[kind]()
        res = {"fit": _attempt(lambda: model.fit(data, **kwargs) and "ok")}
        if stub:
            res["calls"] = list(ctx_cls.log)
        if res["fit"] == "ok":
            res["attributes"] = {k: v for k, v in vars(model).items() if not k.startswith("_predict") and k != "_uploaded"}
            if stub:
                model._predict_ctx = FakePredictCtx()
            for call, method, args, kw in _predict_calls(kind, data):
                res["predict/" + call] = _attempt(lambda: getattr(model, method)(*args, **kw))
            if not stub and model._predict_ctx is not None:
                model._predict_ctx.close()
            model._predict_ctx = None
        out[name] = res
        print(f"  {name}: fit {res['fit'] if isinstance(res['fit'], str) else res['fit'][1]}", flush=True)
    with open(dump, "wb") as f:
        pickle.dump(out, f)


# ----------------------------------------------------------------------------- the comparison (parent side)
def _walk(v, path=""):
    if isinstance(v, dict):
        for k in v:
            yield from _walk(v[k], f"{path}/{k}")
    elif isinstance(v, (list, tuple)) and not (len(v) == 3 and isinstance(v[0], str) and v[0] == "EXC"):
        for i, x in enumerate(v):
            yield from _walk(x, f"{path}[{i}]")
    else:
        yield path, v


def _differs(a, b):
    """None if equal, else a description (arrays: differing bytes)."""
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        if not (isinstance(a, np.ndarray) and isinstance(b, np.ndarray)):
            return f"{type(a).__name__} against {type(b).__name__}"
        if a.dtype != b.dtype or a.shape != b.shape:
            return f"{a.dtype}{a.shape} against {b.dtype}{b.shape}"
        if a.dtype == object or a.dtype.kind in "US":
            return None if np.array_equal(a, b) else "contents differ"
        n = int(np.count_nonzero(np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8)
                                 != np.frombuffer(np.ascontiguousarray(b).tobytes(), np.uint8)))
        return f"{n} of {a.nbytes} bytes differ" if n else None
    if type(a) is not type(b):
        return f"{type(a).__name__} {a!r} against {type(b).__name__} {b!r}"
    if isinstance(a, float) and a != a and b != b:
        return None
    return None if a == b else f"{a!r} against {b!r}"


def compare(old, new, say):
    """Lines for every difference; returns (values compared, unaccepted differences, accepted differences)."""
    total = bad = accepted = 0
    for case in old:
        fo, fn = dict(_walk(old[case])), dict(_walk(new[case]))
        for path in sorted(set(fo) | set(fn)):
            if path.endswith("/wall_seconds"):
                continue
            total += 1
            if path not in fo and "/mcmc_info_/" in path:
                accepted += 1
                say(f"  accepted  {case}{path}: new key ({ACCEPTED_NEW_KEYS})")
                continue
            raised_alike = isinstance(fn.get("/fit"), tuple) and fn.get("/fit") == fo.get("/fit")
            if path not in fn and path.startswith("/calls") and raised_alike and not any(p.startswith("/calls") for p in fn):
                accepted += 1
                say(f"  accepted  {case}{path}: {ACCEPTED_EARLIER}")
                continue
            if path not in fo or path not in fn:
                bad += 1
                say(f"  DIFFERS   {case}{path}: only in the {'new' if path in fn else 'parent'} tree")
                continue
            a, b = fo[path], fn[path]
            if isinstance(a, tuple) and isinstance(b, tuple) and a[:2] == b[:2] and ACCEPTED_MESSAGES.get(a[2]) == b[2]:
                accepted += 1
                say(f"  accepted  {case}{path}: {a[1]} wording {a[2]!r} -> {b[2]!r}")
                continue
            why = _differs(a, b)
            if why:
                bad += 1
                say(f"  DIFFERS   {case}{path}: {why}")
    return total, bad, accepted


def _run_child(tree, stub, dump, seconds):
    env = dict(os.environ, BPLHIP_LIB=os.path.join(ROOT, "bpl-next_amd", "bpl", "libbplhip.so"), FIT_AB_TREE=tree)
    cmd = ["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--child", dump] + (["--stub"] if stub else [])
    subprocess.run(cmd, env=env, check=True)   # one child at a time; a failure ends the run here
    with open(dump, "rb") as f:
        return pickle.load(f)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--stub", action="store_true")
    ap.add_argument("--self", dest="self_", action="store_true", help="first compare two runs of the parent tree")
    ap.add_argument("--parent", help="revision whose bpl-next_amd/bpl is the parent (git archive)")
    ap.add_argument("--parent-dir", help="directory holding the parent's bpl/ (instead of git archive)")
    ap.add_argument("--out", help="also write the report here")
    ap.add_argument("--timeout", type=int, default=500, help="seconds per child process")
    ap.add_argument("--child", metavar="DUMP", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not args.child and (args.parent is None) == (args.parent_dir is None):
        ap.error("give exactly one of --parent REV and --parent-dir DIR")
    if args.child:
        sys.path[:0] = [os.environ["FIT_AB_TREE"], os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
        child(args.stub, args.child)
        return 0
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    with tempfile.TemporaryDirectory() as tmp:
        parent = args.parent_dir
        if parent is None:
            parent = os.path.join(tmp, "bpl-next_amd")
            tar = subprocess.run(["git", "-C", ROOT, "archive", args.parent, "bpl-next_amd/bpl"], check=True, capture_output=True)
            subprocess.run(["tar", "-x", "-C", tmp], input=tar.stdout, check=True)
        parent = os.path.abspath(parent)
        say(f"fit_ab: {'stub' if args.stub else 'device'} context; parent = "
            f"{args.parent if args.parent_dir is None else 'unpacked copy'}, new = working tree")
        bad, unpinned = 0, set()
        say("parent tree, run 1")
        old = _run_child(parent, args.stub, os.path.join(tmp, "old.pkl"), args.timeout)
        if args.self_:
            say("parent tree, run 2")
            again = _run_child(parent, args.stub, os.path.join(tmp, "old2.pkl"), args.timeout)
            say("== parent against itself")
            for case in old:
                t, b, _ = compare({case: old[case]}, {case: again[case]}, say)
                say(f"  {case}: {t} values, {b} differ" + ("  (NOT reproducible run to run: not judged below)" if b else ""))
                if b:
                    unpinned.add(case)
        say("working tree")
        new = _run_child(os.path.join(ROOT, "bpl-next_amd"), args.stub, os.path.join(tmp, "new.pkl"), args.timeout)
        say("== parent against working tree")
        for case in old:
            t, b, acc = compare({case: old[case]}, {case: new[case]}, say)
            bad += 0 if case in unpinned else b
            say(f"  {case}: {t} values, {b} differ, {acc} accepted")
        say(f"total: {bad} differences outside the accepted list")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 3 if bad else 0   # (3: differences; any other non-zero status: a child failed)


if __name__ == "__main__":
    sys.exit(main())
