"""Solver front end: ``get_model`` with the reference's signature and semantics, sieve first.

Mirrors mythril/support/model.py:15-62 line for line in behaviour —

* ``lru_cache(maxsize=2**23)`` keyed on (constraints, minimize, maximize,
  enforce_execution_time); UNSAT raises, so it is never cached;
* time budget: ``min(args.solver_timeout, time_handler.time_remaining() - 500)``, and
  ``UnsatError`` when it is not positive (only with ``enforce_execution_time``);
* a Python ``False`` among the constraints raises ``UnsatError``; Python bools are dropped;
* ``args.solver_log``: the query is written as SMT-LIB2 to ``<dir>/<abs(hash(...))>.smt2``
  (smtlib.py prints this package's terms; foreign terms go through the configured
  ``log_writer``, z3's own ``Optimize.sexpr()`` under the plugin).  A query answered by the
  fallback is logged by the fallback itself (the reference's get_model writes the file), so no
  query is written twice and a writer error never escapes ``get_model``;
* sat -> a ``Model``; unknown / unsat -> ``UnsatError``
* ``SolverStatistics``: ``query_count`` / ``solver_time`` stay z3's own counters — the
  reference's ``stat_smt_query`` on ``BaseSolver.check`` (laser/smt/solver/solver.py:47)
  already counts every fallback query, so the front end adds only the ``sieve_*`` counters

— with one change: when there is nothing to optimise (``minimize == maximize == ()``, the
feasibility case of ``Constraints.is_possible`` and the detection modules), the
query first goes to the sieve (sieve.py).  A witness comes back as a sieve ``Model``, re-verified
by the configured verifier: under the plugin, z3 checks the query with every symbol pinned to the
witness (plugin.witness_pins) and the caller gets z3's model in the reference's ``Model``
(plugin.z3_verifier); with no verifier, the sieve ``Model`` itself.  A miss,
an unsupported term, a device error or a failed verification hands the query, unchanged, to the
fallback solver — the reference's own ``get_model`` when installed by the plugin.  With no
fallback configured a miss is reported the way the reference reports a z3 ``unknown``:
``UnsatError``.  Queries with objectives always go to the fallback (transaction sequences in
reports must stay z3 Optimize output, analysis/solver.py:48-96).
"""
from __future__ import annotations

import inspect
import logging
import threading
import time
from collections import OrderedDict
from functools import lru_cache
from pathlib import Path
from typing import Callable, Optional

from .support import SolverStatistics, UnsatError, args, time_handler

log = logging.getLogger(__name__)

_tls = threading.local()
_config = {
    "fallback": None,   # callable(constraints, minimize, maximize, enforce_execution_time)
    "verify": None,     # callable(constraints, model[, timeout_ms=...]) -> verdict (z3 re-check):
                        # falsy rejects, True keeps the sieve Model, another object is the
                        # model returned instead (z3_verifier: the reference's Model); timeout_ms
                        # (what is left of get_model's budget) is passed only to a verifier that
                        # declares it (or **kwargs)
    "to_terms": None,   # callable(constraints) -> (smt.Context, [Bool]) for foreign terms
    "log_writer": None,  # callable(constraints, minimize, maximize) -> SMT-LIB2 text (foreign)
    "fallback_logs": False,  # the fallback writes --solver-log files itself (the reference's)
    "sieve_kwargs": {},
    "enabled": True,
    "certify": None,    # certify every witness against the original constraints (certify.py)
                        # before the verifier sees it; None: the SIEVE_CERTIFY environment
                        # variable ("1" turns it on), off by default
    "certify_resident": None,  # sieve_model's own certification goes through the sieve's
                               # resident Certifier (certify.py); None: SIEVE_CERTIFY_RESIDENT=1
                               # turns it on, off by default
    "decide": None,     # what a query the sieve decided UNSAT (Sieve.last_unsat; needs the sieve
                        # option decide_rows) becomes: False / off -- a miss like any other;
                        # True -- UnsatError without the fallback; "audit" -- the fallback is
                        # still asked and a model it returns is counted as a dispute.  None: the
                        # SIEVE_DECIDE environment variable ("1" / "audit"), off by default
}


class SieveUnavailable(RuntimeError):
    """This thread's sieve could not be created (no library, no gfx950 device); the message
    is the original failure's."""


def configure(*, fallback: Optional[Callable] = None, verify: Optional[Callable] = None,
              to_terms: Optional[Callable] = None, enabled: Optional[bool] = None,
              log_writer: Optional[Callable] = None, fallback_logs: Optional[bool] = None,
              certify: Optional[bool] = None, certify_resident: Optional[bool] = None,
              decide=None, **sieve_kwargs) -> None:
    """Set the fallback solver, the witness verifier, the term importer and sieve options.
    ``certify=True`` (or SIEVE_CERTIFY=1) certifies every witness against the original
    constraints on the device before it is returned or verified (certify.py);
    ``certify_resident=True`` (or SIEVE_CERTIFY_RESIDENT=1) does so through the sieve's resident
    Certifier, which keeps a path's compiled constraints between queries.
    ``decide`` (or SIEVE_DECIDE) says what a query the sieve decided UNSAT by enumeration becomes
    (decide_mode); the decisions themselves are switched on by the sieve option ``decide_rows``.
    Sieve options (``rows``, ``spares``, ``batch_spares``, ...) are further keywords, or one dict
    ``sieve_kwargs``; with ``spares`` and ``batch_spares`` the batched first rounds of ``prefetch``
    try the ancestors' spare rows and store spares too."""
    if decide is not None:
        if decide not in (True, False, "audit"):
            raise ValueError("decide must be True, False or 'audit'")
        _config["decide"] = decide
    if certify is not None:
        _config["certify"] = bool(certify)
    if certify_resident is not None:
        _config["certify_resident"] = bool(certify_resident)
    if fallback is not None:
        _config["fallback"] = fallback
    if log_writer is not None:
        _config["log_writer"] = log_writer
    if fallback_logs is not None:
        _config["fallback_logs"] = fallback_logs
    if verify is not None:
        _config["verify"] = verify
    if to_terms is not None:
        _config["to_terms"] = to_terms
    if enabled is not None:
        _config["enabled"] = enabled
    nested = sieve_kwargs.pop("sieve_kwargs", None)  # the options as one dict, as _config keeps them
    if nested:
        sieve_kwargs.update(nested)
    if sieve_kwargs:
        _config["sieve_kwargs"] = dict(sieve_kwargs)
        close_sieve()
    clear_prefetched()
    get_model.cache_clear()


def certification_on() -> bool:
    """configure(certify=...) when set, else SIEVE_CERTIFY=1; off by default."""
    import os

    c = _config["certify"]
    return os.environ.get("SIEVE_CERTIFY", "") == "1" if c is None else c


def certify_resident_on() -> bool:
    """configure(certify_resident=...) when set, else SIEVE_CERTIFY_RESIDENT=1; off by default."""
    import os

    c = _config["certify_resident"]
    return os.environ.get("SIEVE_CERTIFY_RESIDENT", "") == "1" if c is None else c


def decide_mode():
    """False (the default: a decided-UNSAT query is a miss like any other), True (it raises
    UnsatError without the fallback) or "audit" (the fallback is still asked, and a model it
    returns is a dispute): configure(decide=...) when set, else SIEVE_DECIDE ("1" / "audit")."""
    import os

    d = _config["decide"]
    if d is None:
        e = os.environ.get("SIEVE_DECIDE", "")
        d = True if e == "1" else "audit" if e == "audit" else False
    return d


def _takes_timeout(fn) -> bool:
    try:
        ps = inspect.signature(fn).parameters.values()
    except (TypeError, ValueError):
        return False
    return any(p.name == "timeout_ms" or p.kind == p.VAR_KEYWORD for p in ps)


def _verify(verify, constraints, m, left):
    """The verifier's verdict: falsy rejects; True accepts the sieve's Model; any other object
    is the model to return instead (plugin.z3_verifier: the reference's Model of z3's check)."""
    if _takes_timeout(verify):
        return verify(constraints, m, timeout_ms=left)
    return verify(constraints, m)


def reset() -> None:
    """Back to defaults (tests, plugin stop)."""
    _config.update(fallback=None, verify=None, to_terms=None, log_writer=None,
                   fallback_logs=False, sieve_kwargs={}, enabled=True, certify=None,
                   certify_resident=None, decide=None)
    close_sieve()
    clear_prefetched()
    get_model.cache_clear()


def sieve():
    """This thread's sieve (device context + buffers), created on first use.  A failure to
    create it (no library, no gfx950 device) is remembered: later queries go straight to the
    fallback without importing their terms or probing the device again, until the sieve is
    reconfigured (configure with sieve options, reset)."""
    s = getattr(_tls, "sieve", None)
    if s is None:
        failed = getattr(_tls, "sieve_failed", None)
        if failed is not None:
            # a fresh exception per query: re-raising one saved object would chain every
            # query's frames (and their constraints) onto its traceback
            raise SieveUnavailable(failed)
        from .sieve import Sieve

        try:
            s = _tls.sieve = Sieve(**_config["sieve_kwargs"])
        except Exception as e:
            _tls.sieve_failed = "%s: %s" % (type(e).__name__, e)
            log.warning("constraint sieve unavailable, every query goes to the fallback: %s", e)
            raise
    return s


def _forget(s, key) -> None:
    """A rejected witness leaves the sieve, with the spare models stored beside it."""
    forget = getattr(s, "forget", None)
    if forget is not None:
        forget(key)
    else:  # a stand-in without the method
        s.witnesses.pop(key, None)


def forget_witnesses() -> None:
    """Drop the sieve's parent-witness table (its keys are node ids of a term context the
    importer has just replaced)."""
    s = getattr(_tls, "sieve", None)
    if s is not None:
        s.witnesses.clear()
        getattr(s, "spare_witnesses", {}).clear()
    clear_prefetched()  # (keyed by the same node ids)


def close_sieve() -> None:
    s = getattr(_tls, "sieve", None)
    if s is not None:
        s.close()
        _tls.sieve = None
    _tls.sieve_failed = None


def _log_query(constraints, minimize, maximize) -> None:
    """support/model.py:44-55: one ``.smt2`` file per query, named by the hash of the query.
    This package's terms print through smtlib.to_smtlib; foreign (z3) terms through the
    configured ``log_writer``.  Never raises: a query that cannot be printed is skipped (the
    reference only logs what z3 can print, and a log must not change the answer)."""
    from . import smt

    try:
        if all(isinstance(c, smt.Bool) for c in constraints) and \
                all(isinstance(e, smt.BitVec) for e in tuple(minimize) + tuple(maximize)):
            from .smtlib import to_smtlib

            text = to_smtlib(constraints, minimize, maximize)
        elif _config["log_writer"] is not None:
            text = _config["log_writer"](constraints, minimize, maximize)
        else:
            log.debug("--solver-log: no writer for %s terms", type(constraints[0]).__name__)
            return
        Path(args.solver_log).mkdir(parents=True, exist_ok=True)
        key = tuple(list(constraints) + list(minimize) + list(maximize)
                    + [len(constraints), len(minimize), len(maximize)])
        with open(args.solver_log + "/%d.smt2" % abs(hash(key)), "w") as f:
            f.write(text)
    except Exception as e:  # noqa: BLE001 - logging is best effort
        log.debug("--solver-log write failed: %s", e)


def _query_text(constraints) -> str:
    """The query as SMT-LIB2 for a log message (a disputed decision), best effort."""
    from . import smt

    try:
        if all(isinstance(c, smt.Bool) for c in constraints):
            from .smtlib import to_smtlib

            return to_smtlib(constraints, (), ())
        if _config["log_writer"] is not None:
            return _config["log_writer"](constraints, (), ())
    except Exception:  # noqa: BLE001 - a message must not change the answer
        pass
    return repr(constraints)


def _terms(constraints):
    """(smt.Context, [Bool]) for the constraints: ours as they are, foreign ones imported."""
    from . import smt

    if all(isinstance(c, smt.Bool) for c in constraints):
        ctx = constraints[0].ctx if constraints else smt.context()
        if any(c.ctx is not ctx for c in constraints):
            raise ValueError("constraints from different term contexts")
        return ctx, list(constraints)
    conv = _config["to_terms"]
    if conv is None:
        raise TypeError("no importer for constraints of type %s"
                        % type(constraints[0]).__name__)
    return conv(constraints)


PARKED_MAX = 4096  # answers prefetch() keeps per thread, oldest dropped


def _parked() -> "OrderedDict":
    """This thread's parked answers (prefetch): key -> (term context, witness or None, the
    sieve's last_miss, its last_rounds)."""
    t = getattr(_tls, "parked", None)
    if t is None:
        t = _tls.parked = OrderedDict()
    return t


def _parked_verdicts() -> dict:
    """This thread's parked verdicts (prefetch with certification on): key -> (term context,
    certify_many's entry for the parked witness).  Cleared with the parked answers."""
    t = getattr(_tls, "parked_verdicts", None)
    if t is None:
        t = _tls.parked_verdicts = {}
    return t


def clear_prefetched() -> None:
    """Drop this thread's parked answers (configure, reset, forget_witnesses do)."""
    for name in ("parked", "parked_verdicts", "parked_unsat"):
        t = getattr(_tls, name, None)
        if t:
            t.clear()


def prefetch(queries) -> int:
    """Solve many feasibility queries ahead of the get_model calls that will ask them, with
    their first rounds in one device submission (Sieve.solve_many): ``queries`` is an iterable of
    constraint tuples, as get_model takes them -- LASER asks every open world state's
    constraints at the start of a transaction round (laser/ethereum/svm.py:201-203).  Each
    answer is parked under the query's key; sieve_model looks there before it runs a round of
    its own: a parked witness goes through certification and the verifier as any other, a parked
    miss goes to the fallback without a device round (and the fallback's model is still
    learnt).  With certification on, the witnesses found are certified here in one
    Certifier.certify_many and each verdict is parked beside its answer: sieve_model then uses it
    instead of certifying again (the counters move there, as they do today); a rejected witness
    is dropped from the sieve's parent-witness table at once.  If that certification errors, the
    answers stay parked without verdicts and take the ordinary path.  A query with a Python False is UNSAT without the sieve and is skipped; other bools
    are dropped, as in get_model.  The whole list shares args.solver_timeout.  Never raises: any
    error leaves the table as it was and the queries to the ordinary path.  Returns the number
    of answers parked."""
    try:
        if not _config["enabled"]:
            return 0
        s = sieve()
        table = _parked()
        items, seen = [], set()
        for q in queries:
            cs = tuple(q)
            if any(type(c) == bool and not c for c in cs):
                continue
            cs = [c for c in cs if type(c) != bool]
            if not cs:
                continue
            ctx, terms = _terms(cs)
            key = tuple(t.node for t in terms)
            if key in seen or (key in table and table[key][0] is ctx):
                continue
            seen.add(key)
            items.append((ctx, key))
        # (an importer that replaced its term context on the way has made the earlier keys stale)
        items = [it for it in items if it[0] is items[-1][0]]
        if not items:
            return 0
        out = s.solve_many([ctx.b for ctx, _ in items], [list(key) for _, key in items],
                           keys=[key for _, key in items],
                           budget_s=max(args.solver_timeout, 0.0) / 1000.0)
        fresh = [(key, (ctx, w, rec["miss"], rec["rounds"]))
                 for (ctx, key), w, rec in zip(items, out, s.last_many) if rec["error"] is None]
    except Exception as e:  # noqa: BLE001 - prefetching never changes an answer
        log.debug("prefetch left to the ordinary path: %s", e)
        return 0
    verdicts = _parked_verdicts()
    unsat = getattr(_tls, "parked_unsat", None)
    if unsat is None:
        unsat = _tls.parked_unsat = set()
    for (_, key), rec in zip(items, s.last_many):  # the parked misses that were decisions
        if rec["error"] is None:
            (unsat.add if rec.get("unsat") else unsat.discard)(key)
    for key, entry in fresh:
        table[key] = entry
        table.move_to_end(key)
        verdicts.pop(key, None)
    if certification_on():
        verdicts.update(_certify_parked(s, fresh))
    while len(table) > PARKED_MAX:
        verdicts.pop(table.popitem(last=False)[0], None)
    return len(fresh)


def _certify_parked(s, fresh) -> dict:
    """key -> (term context, verdict) for the witnesses among the freshly parked answers: one
    Certifier.certify_many for all of them.  Never raises: on an error nothing is verdicted."""
    from .model import Model

    found = [(key, e) for key, e in fresh if e[1] is not None]
    if not found:
        return {}
    conv = _config["to_terms"]
    importer = conv if hasattr(conv, "term") else None
    try:
        models = [Model(s, ctx, w.schema, w.values, w.index, importer=importer)
                  for _, (ctx, w, _, _) in found]
        got = s.certifier().certify_many(models, [list(key) for key, _ in found])
    except Exception as e:  # noqa: BLE001 - the witnesses are certified one by one later
        log.debug("prefetch: certification left to the ordinary path: %s", e)
        return {}
    out = {}
    for (key, (ctx, _, _, _)), v in zip(found, got):
        out[key] = (ctx, v)
        if not isinstance(v, Exception) and not v:
            _forget(s, key)  # does not seed the query's children
    return out


def sieve_model(constraints, timeout_ms: Optional[float] = None):
    """The sieve's answer for a feasibility query: a Model, or None (ask the fallback).
    ``timeout_ms`` is get_model's budget (support/model.py:26-31): the sieve's own rounds and the
    verifier both stop inside it."""
    from .model import Model

    stats = SolverStatistics()
    t0 = time.perf_counter()
    _tls.miss_key = None
    _tls.decided_unsat = False  # this call's miss was a decision (get_model reads it)
    try:
        s = sieve()  # first: an unusable device skips the term import
        ctx, terms = _terms(constraints)
        key = tuple(t.node for t in terms)
        budget = None if timeout_ms is None else max(timeout_ms, 0.0) / 1000.0
        parked = getattr(_tls, "parked", None)
        entry = parked.pop(key, None) if parked else None
        pv = getattr(_tls, "parked_verdicts", None)
        pv = pv.pop(key, None) if pv else None
        parked_verdict = None
        if entry is not None and entry[0] is ctx and pv is not None and pv[0] is ctx:
            parked_verdict = pv[1]
        if entry is not None and entry[0] is ctx:
            # answered by prefetch(): no round here; a miss leaves the sieve as solve() would
            # have, so the fallback's model of it is learnt
            _, w, s.last_miss, s.last_rounds = entry
            pu = getattr(_tls, "parked_unsat", None)
            unsat = bool(pu) and key in pu
            if unsat:
                pu.discard(key)
        else:
            w = s.solve(ctx.b, [t.node for t in terms], key=key, budget_s=budget)
            unsat = bool(getattr(s, "last_unsat", False))
        _tls.decided_unsat = w is None and unsat
    except Exception as e:  # fail closed: any problem means "ask the fallback"
        from .lower import LoweringUnsupported
        from .native import Unsupported

        if isinstance(e, (LoweringUnsupported, Unsupported)):
            stats.sieve_unsupported += 1
        else:
            stats.sieve_errors += 1
            log.debug("sieve error: %s", e)
        return None
    if w is None:
        stats.sieve_misses += 1
        _tls.miss_key = key  # the fallback's model of this query is learnt (learn_from_fallback)
        _tls.miss_ctx = ctx
        return None
    conv = _config["to_terms"]  # reads reference terms for Model.eval / Model[decl]
    m = Model(s, ctx, w.schema, w.values, w.index,
              importer=conv if hasattr(conv, "term") else None)
    if certification_on():
        # the original constraints under the model's extensional meaning, on the device; a
        # witness that fails, or one the certifier cannot judge, is handled like a verifier's
        # rejection, and is dropped from the sieve so it does not seed this query's children
        from .certify import CertifyUnsupported, certify
        from .native import Unsupported

        try:
            if parked_verdict is not None:  # certified by prefetch(), with the other answers
                if isinstance(parked_verdict, Exception):
                    raise parked_verdict
                verdict = parked_verdict
            elif certify_resident_on():
                verdict = s.certifier().certify(m, terms)
            else:
                verdict = certify(m, terms)
        except (CertifyUnsupported, Unsupported) as e:
            stats.sieve_uncertified += 1
            log.debug("sieve witness not certified: %s", e)
            verdict = False
        except Exception as e:  # noqa: BLE001 - a device or ABI error says nothing about the
            # witness: an error, not a rejection (fail closed: the query goes to the fallback)
            stats.sieve_errors += 1
            log.debug("sieve witness certification error: %s", e)
            return None
        if not verdict:
            if verdict is not False:
                log.debug("sieve witness rejected by certification: %r", verdict)
            stats.sieve_rejected += 1
            _forget(s, key)
            return None
    verify = _config["verify"]
    if verify is not None:
        left = None if timeout_ms is None else timeout_ms - 1000.0 * (time.perf_counter() - t0)
        try:
            ok = left is None or left > 0
            ok = ok and _verify(verify, constraints, m, left)
        except Exception as e:  # noqa: BLE001 - a failing verifier rejects
            log.debug("sieve witness verifier error: %s", e)
            ok = False
        if not ok:
            stats.sieve_rejected += 1
            return None
        if ok is not True:
            m = ok  # the verifier's own model (the reference's type)
    stats.sieve_hits += 1
    return m


@lru_cache(maxsize=2 ** 23)
def get_model(constraints, minimize=(), maximize=(), enforce_execution_time=True):
    """support/model.py:15-62 with the sieve in front of the solver (module docstring)."""
    timeout = args.solver_timeout
    if enforce_execution_time:
        timeout = min(timeout, time_handler.time_remaining() - 500)
        if timeout <= 0:
            raise UnsatError
    for constraint in constraints:
        if type(constraint) == bool and not constraint:
            raise UnsatError
    constraints = [c for c in constraints if type(c) != bool]
    stats = SolverStatistics()
    fallback = _config["fallback"]
    _tls.miss_key = None  # set by this call's sieve miss only
    if _config["enabled"] and not minimize and not maximize:
        t0 = time.perf_counter()
        m = sieve_model(constraints, timeout)
        if stats.enabled:
            stats.sieve_time += time.perf_counter() - t0
        if m is not None:
            if args.solver_log:
                _log_query(constraints, minimize, maximize)
            return m
    # a miss that was a decision (Sieve.last_unsat: an eligible group enumerated to its end, or
    # an eligible query the host refuted), under decide=True / "audit"
    mode = decide_mode() if getattr(_tls, "decided_unsat", False) else False
    _tls.decided_unsat = False
    if mode:
        stats.sieve_unsat += 1
    if args.solver_log and (fallback is None or not _config["fallback_logs"] or mode is True):
        _log_query(constraints, minimize, maximize)
    if mode is True:  # the sieve's own UNSAT: the fallback is not asked
        raise UnsatError
    if fallback is None:
        log.debug("sieve found no witness and no fallback solver is configured")
        raise UnsatError
    # the fallback (the reference's get_model) counts itself through stat_smt_query
    model = fallback(tuple(constraints), minimize, maximize, enforce_execution_time)
    if mode == "audit" and model is not None:
        stats.sieve_unsat_disputed += 1
        log.warning("sieve decided UNSAT, the fallback found a model: %s",
                    _query_text(constraints))
    learn_from_fallback(model)
    return model


def z3_column_reader(model, z3):
    """value_of(column) over a z3 model -- the reference's Model (laser/smt/model.py:12-59: its
    ``raw`` z3 ModelRefs) or a z3 ModelRef -- for Sieve.learn: a variable's value, an array cell
    ``Select(A, key)``, a function cell ``f(key)``, each evaluated with model completion; None
    for the else columns (any value completes a model) and for symbols the model does not
    declare.  ``value_of.value_at(column, index)`` reads a read column (``Select(A, i)``,
    ``f(i)``, keccak included) at its index term's value, which Sieve.learn computes."""
    models = list(getattr(model, "raw", None) or [model])
    decls = {}
    for zm in models:
        for d in zm.decls():
            decls.setdefault(d.name(), (zm, d))

    def at(col, key):
        hit = decls.get(col.symbol)
        if hit is None:
            return None
        zm, d = hit
        if col.kind == "var":
            v = zm.eval(d(), model_completion=True)
        elif col.kind in ("cell", "read"):
            v = zm.eval(z3.Select(d(), z3.BitVecVal(key, d.range().domain().size())),
                        model_completion=True)
        else:
            v = zm.eval(d(z3.BitVecVal(key, d.domain(0).size())), model_completion=True)
        return v.as_long() if z3.is_bv_value(v) else None

    def value_of(col):
        if col.kind not in ("var", "cell", "ufcell"):
            return None
        return at(col, col.key)

    def value_at(col, index):
        """A read column (an array's, a tabled function's or a keccak function's value at a
        symbolic index term) at that term's value ``index`` (Sieve.learn computes it)."""
        if col.kind not in ("read", "ufread", "kread"):
            return None
        return at(col, index)

    value_of.value_at = value_at
    return value_of


def learn_from_fallback(model) -> None:
    """The fallback's model of the query the sieve just missed becomes that query's witness in
    the sieve (Sieve.learn), so the query's children are generated around it.  Best effort: no
    z3, a model of another shape or any error leaves the sieve as it was."""
    key = getattr(_tls, "miss_key", None)
    _tls.miss_key = None
    s = getattr(_tls, "sieve", None)
    if key is None or s is None or model is None:
        return
    try:
        import z3

        reader = z3_column_reader(model, z3)
        s.learn(key, reader, ctx=getattr(_tls, "miss_ctx", None), value_at=reader.value_at)
    except Exception as e:  # noqa: BLE001 - learning never changes the answer
        log.debug("fallback model not learnt: %s", e)
