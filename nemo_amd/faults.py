"""Fault events over a corpus's interned labels, as candidates for Engine.min_group_cuts (host only).

Molly injects two kinds of fault (nemo_amd/molly/ldfi.py, `_events` and `kills`): the omission of one message, which
removes one clock goal, and the crash of a node n at time t, which removes every clock goal n would send from t on
and every one it would receive at t or later.  A clock goal is the same interned label in every run of a corpus, so a
fault event is a set of labels: a candidate group of nemo_min_group_cuts.  "One crash plus one omission" is then a pair
of candidates, and the device search names it without a round trip.
"""
from __future__ import annotations

import re
from typing import List, Sequence, Tuple

WILD = "__WILDCARD__"  # nemo_amd.molly.dedalus.WILD as the labels spell it: clock(n, n, t, __WILDCARD__)
_CLOCK = re.compile(r"^clock\((.*)\)$")

Event = Tuple[str, str, object, int]  # ("omit", from, to, t) | ("crash", node, None, t)


def parse_clock(label: str):
    """(from, to, send time, wildcard?) of a clock label `clock(f, d, t, t+1)` / `clock(n, n, t, __WILDCARD__)`, or
    None for every other label (another table, another arity, a send time that is no integer)."""
    m = _CLOCK.match(label.strip())
    if not m:
        return None
    parts = [p.strip() for p in m.group(1).split(",")]
    if len(parts) != 4:
        return None
    try:
        t = int(parts[2])
    except ValueError:
        return None
    return parts[0], parts[1], t, parts[3] == WILD


def fault_events(labels: Sequence[str], eot: int, eff: int) -> Tuple[List[Event], List[List[int]]]:
    """The fault events of a corpus and their label groups, by ldfi.py's rule.

    labels: the corpus's label strings (Corpus.labels), label id = index.  eot / eff: the run's end of time and end
    of finite failures (runs.json's failureSpec).  Returns (events, groups), of equal length; groups[k] holds the
    label ids event k removes, ascending, each once.  The order is fixed:

    * first the omissions ("omit", f, d, t), one per label `clock(f, d, t, t+1)` with f != d and t < eff, sorted by
      (t, f, d); the group is that single label;
    * then the crashes ("crash", n, None, t) for every node n seen in a clock label (as sender or receiver), in
      sorted order, and t = 1 .. eot ascending; the group holds every clock label with sender n and send time >= t,
      the __WILDCARD__ form included, and every non-wildcard clock label with receiver n and send time + 1 >= t.

    Labels that are no clock goals belong to no group.  A crash group may be empty (nothing left to send or receive
    at t): it stays in the list, so that positions depend on the nodes and eot alone; the search never makes an
    empty group live.

    A crash budget (at most c distinct crashed nodes, Molly's maxCrashes) is the caller's filter over the returned
    rows: drop the rows whose events crash more than c nodes.  That is sound, because every subset of a set within
    the budget is within the budget: a row within budget that is minimal among all candidate sets has no proper
    subset that is a cut, in budget or not, so it is also minimal among the sets within budget; and a set within
    budget that is a cut and minimal among those has only subsets within budget, none of them a cut, so it is
    minimal among all sets and is a returned row.
    """
    clocks = []  # (label id, f, d, t, wildcard)
    nodes = set()
    for lid, s in enumerate(labels):
        c = parse_clock(s)
        if c is None:
            continue
        f, d, t, wild = c
        clocks.append((lid, f, d, t, wild))
        nodes.add(f)
        if not wild:
            nodes.add(d)
    events: List[Event] = []
    groups: List[List[int]] = []
    for t, f, d, lid in sorted((t, f, d, lid) for lid, f, d, t, wild in clocks if not wild and f != d and t < eff):
        events.append(("omit", f, d, t))
        groups.append([lid])
    for n in sorted(nodes):
        for ct in range(1, eot + 1):
            g = sorted({lid for lid, f, d, t, wild in clocks if (f == n and t >= ct) or (not wild and d == n and t + 1 >= ct)})
            events.append(("crash", n, None, ct))
            groups.append(g)
    return events, groups
