"""What the stash audit and the trunk audit share (DESIGN.md section 6j "census core"): when an audit is due, why one is refused, how
an entry of a census record is read, when a report is flagged and how the reports are written."""
import collections
import json

import torch

from ._lib import CENSUS_FIELDS, CENSUS_BINS


class AuditSchedule:
    """One audit kind of one fit: every (N > 0: each N-th iteration, 0: never), armed (the next iteration that records), reports (a
    deque of the last maxlen reports: the oldest go first) and last (the newest report, None before the first)."""

    def __init__(self, every, maxlen):
        self.every, self.armed, self.reports, self.last = int(every), False, collections.deque(maxlen=maxlen), None

    def arm(self):
        self.armed = True

    def due(self, iteration):
        return self.armed or (self.every > 0 and iteration % self.every == 0)

    def record(self, rep):
        self.armed, self.last = False, rep
        self.reports.append(rep)
        return rep


def _stash_conditions(me, flag, precision, **_):
    from .ops import tune
    yield precision != "bf16", (f"{me} with {'--precision ' + precision if flag else 'precision=' + repr(precision)}: the exact-fp32 chain has no "
                                f"8-bit stash (its stash is fp32, nothing is rounded)")
    yield not tune("stash8"), f"{me} with {'NPP_STASH8=0 / ' if flag else ''}npp_tune('stash8') = 0: the 16-bit stash is in use, there is nothing to audit"


def _trunk_conditions(me, flag, trunk_precision, patch_losses=True, stacked=False, **_):
    yield stacked, (f"{me}: stacked fits share one launch sequence and cannot be audited; "
                    f"{'drop --stack or --audit_trunk' if flag else 'pass fits built with trunk_audit=0'}")
    yield trunk_precision != "fp16", (f"{me} with {'--trunk_precision ' + str(trunk_precision) if flag else 'trunk_precision=' + repr(trunk_precision)}: "
                                      f"the trunks already run in exact fp32, there is nothing 16-bit to audit")
    yield not patch_losses, (f"{me} on a fit without patch losses ({'no periodicity shifts were found' if flag else 'shifts=None'}): no VGG trunk "
                             f"runs, there is nothing to audit")


# kind: (the command line's flag, the Python interface's name, what the audit reads back, its conditions)
_REFUSALS = {"stash": ("--audit_stash", "stash audit", "record", _stash_conditions),
             "trunk": ("--audit_trunk", "trunk audit (trunk_audit)", "records", _trunk_conditions)}


def refuse(kind, exc=ValueError, flag=False, capturing=None, **state):
    """Refuse an audit by name where it has nothing to audit (the kind's conditions, each taking what it needs of `state`) and while
    a stream capture is open (an audit copies what it counted to the host).  exc: ValueError for the Python interface, SystemExit
    for the command line; flag: name the switches as flags; capturing None: ask the current stream."""
    flag_name, name, reads, conditions = _REFUSALS[kind]
    me = flag_name if flag else name
    for hit, text in conditions(me, flag, **state):
        if hit:
            raise exc(text)
    if capturing is None:
        capturing = torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()
    if capturing:
        raise exc(f"{me} while a stream capture is open: an audit reads its {reads} back on the host; run it outside "
                  f"torch.cuda.graph / hipStreamBeginCapture")


def decode_entry(rec, off=0):
    """One entry of a census record (int64 NumPy) at word `off`: the five counters, then "exp_hist": the 32 exponent bins."""
    e = {f: int(rec[off + i]) for i, f in enumerate(CENSUS_FIELDS)}
    e["exp_hist"] = [int(v) for v in rec[off + len(CENSUS_FIELDS):off + len(CENSUS_FIELDS) + CENSUS_BINS]]
    return e


def at_limits(entries):
    """(codes at their format's largest finite value, non-finite codes) over decoded entries."""
    entries = list(entries)
    return tuple(sum(e[k] for e in entries) for k in ("at_max", "nonfinite"))


def saturated(entries):
    """Exact: some decoded entry holds a code at its format's largest finite value or a non-finite one."""
    return sum(at_limits(entries)) > 0


def audit_dumps(key, reports, fmt):
    """An audit's JSON file: [{key: fmt}, report, report, ...]; json.loads gives the reports back."""
    return json.dumps([{key: fmt}] + [dict(r) for r in reports], indent=1)
