"""The scheduling core of the main-loop body generators (tools/gen_*_body.py): nothing of any one kernel lives here.

A generator describes one body of its kernel's main loop as a list of MFMAs (text, the keys of the LDS reads it consumes)
and a list of filler Tasks (LDS reads, VALU work, vector-memory operations) with a release gap, a deadline gap and
dependencies, in units of "the gap behind MFMA number g".  From that the core makes the text of one asm statement:

    place()         every task into a gap, earliest deadline first, within an issue budget per gap
    render_lines()  the body in issue order, with the counted `s_waitcnt lgkmcnt(n)` in front of each MFMA derived from the
                    steady-state order of the LDS operations.  Bodies are CYCLIC: tasks placed into negative gaps are
                    emitted in the tail of the previous body, tagged '@N ', with the next body's addresses.
    resolve()       the @KEY+offset placeholders of a rendered body to numbers, for one (buffer, sub-tile, ...) instance
    main()          the command line every generator has: --check prints the schedule's load, --out names the file

Nothing here reads the environment or keeps state between calls: each generator reads its own FA2_GEN_* switches and hands
the values down as arguments, so any number of generators can run in one interpreter.
"""
import argparse
import os
import re

GAP_BUDGET = 20          # clocks of other issue hidden per MFMA (one wave per SIMD)
COST = {"lds": 4, "valu": 4, "exp": 8, "cvt": 4, "mask": 16}
READ_AHEAD = 7           # issue a fragment read this many MFMAs before its consumer ...
READ_LATEST = 4          # ... and not later than this many
WAIT_AGE = 3
WAIT_LOOK = 0            # see render_lines; 2 was MEASURED 2-3 % slower (fused backward)
BARRIER = ["s_waitcnt vmcnt(0)", "s_barrier"]


class Task:
    __slots__ = ("text", "cost", "release", "deadline", "kind", "key", "gap", "seq", "after")

    def __init__(self, text, cost, release, deadline, kind, key=None, after=None):
        self.text, self.cost, self.release, self.deadline, self.kind, self.key = text, cost, release, deadline, kind, key
        self.after = after or []       # tasks that must be placed (strictly earlier in issue order) before this one
        self.gap = None


def prune(tasks, mfma, gone):
    """The ablations (timing only, wrong results): (tasks, mfma) without the tasks for which gone(task) holds -- nobody
    waits for them any more, neither a surviving task (`after`) nor an MFMA (`needs`)."""
    dead = set(id(t) for t in tasks if gone(t))
    tasks = [t for t in tasks if id(t) not in dead]
    for t in tasks:
        t.after = [d for d in t.after if id(d) not in dead]
    present = set(t.key for t in tasks)
    return tasks, [(text, [k for k in needs if k in present]) for text, needs in mfma]


def place(tasks, NS, budget=GAP_BUDGET):
    """Places every task into a gap (possibly negative = previous body), earliest deadline first, respecting the
    dependencies in `after`.  Returns (per-gap lists in issue order, per-gap load)."""
    load = {}
    for i, t in enumerate(tasks):
        t.seq = i
    # LDS reads are placed FIRST, on their own: which of them a body leaves in flight for the next one (the tasks with
    # negative gaps) must not depend on the VALU load, because plain and masked bodies follow each other in any order.
    for phase in (0, 1):
        pending = sorted((t for t in tasks if (t.kind == "lds") == (phase == 0)), key=lambda t: (t.deadline, t.seq))
        guard = 0
        while pending:
            guard += 1
            assert guard < 100000
            progressed = False
            for t in list(pending):
                lo = t.release
                ok = True
                for dep in t.after:
                    if isinstance(dep, tuple):           # ("prev", task): the dependency sits in the PREVIOUS body
                        d = dep[1]
                        if d.gap is None:
                            ok = False
                            break
                        lo = max(lo, d.gap - NS + 1)
                    else:
                        if dep.gap is None:
                            ok = False
                            break
                        lo = max(lo, dep.gap + (1 if dep.kind == "exp" else 0))    # a trans result is not read in the same gap
                if not ok:
                    continue
                g = lo
                while load.get(g % NS, 0) + t.cost > budget and g < t.deadline:
                    g += 1
                assert g <= t.deadline, (t.text, g, t.deadline)
                t.gap = g
                load[g % NS] = load.get(g % NS, 0) + t.cost
                pending.remove(t)
                progressed = True
            assert progressed, "dependency cycle (an LDS task may not depend on a VALU task)"
    per_gap = {}
    for t in tasks:
        per_gap.setdefault(t.gap, []).append(t)
    for g in per_gap:
        per_gap[g].sort(key=lambda t: (0 if t.kind == "lds" else 1, t.seq))
    return per_gap, [load.get(g, 0) for g in range(NS)]


def render_lines(mfma, per_gap, NS, wait_look=WAIT_LOOK, wait_age=WAIT_AGE, lds_writes=False):
    """(body lines with @placeholders, prologue lines) of a cyclic schedule.  Lines tagged '@N ' belong to the NEXT
    body's early work (they use the next unit's bases); the counted lgkmcnt in front of each MFMA is derived from the
    steady-state issue order of the LDS operations (two periods are simulated, the second one is emitted).  With
    lds_writes, tasks of kind 'ldsw' are counted in that order too (LDS writes share lgkmcnt and return in order)."""
    in_order = ("lds", "ldsw") if lds_writes else ("lds",)
    gmin = min(per_gap)
    assert gmin >= -NS, gmin

    def gap_items(g):
        own = per_gap.get(g, []) if g >= 0 else []
        nxt = per_gap.get(g - NS, []) if g - NS < 0 else []
        return own, nxt

    issued = []         # keys in issue order; entries are (period, key)
    issue_gap = []      # absolute gap (period * NS + g) at which each was issued
    waited_upto = [-1]  # index into `issued` up to which completion is known
    lines = []
    for period in (0, 1):
        for g in range(NS):
            text, needs = mfma[g]
            pos = -1
            for k in needs:
                idx = max(i for i, (p, kk) in enumerate(issued) if kk == k and p == period) if any(kk == k and p == period for p, kk in issued) else None
                assert idx is not None or period == 0, (k, g)
                if idx is not None:
                    pos = max(pos, idx)
            cnt = min(len(issued) - 1 - pos, 15) if pos >= 0 else None
            # a wait is needed only if it asks for something an earlier wait has not already covered (LDS returns in order)
            if cnt is not None and len(issued) - 1 - cnt <= waited_upto[0]:
                cnt = None
            if cnt is not None and wait_look:
                # fewer s_waitcnt: one wait may also cover what the next wait_look MFMAs need, as far as those reads have been
                # in flight for wait_age MFMAs.  Without the age limit it halves the waits and is 2-3 % SLOWER (the merged
                # wait stalls on reads issued a moment ago); with it, about 1 % faster in the fused backward, which sets
                # its own values.  Off (0) for the dQ and dK/dV bodies.
                for g2 in range(g + 1, g + 1 + wait_look):
                    p2 = period + g2 // NS
                    for k in mfma[g2 % NS][1]:
                        hits = [i for i, (p, kk) in enumerate(issued) if kk == k and p == p2]
                        # only reads that have been in flight for wait_age MFMAs or more: younger ones may not have landed
                        if hits and issue_gap[hits[-1]] <= period * NS + g - wait_age:
                            pos = max(pos, hits[-1])
                cnt = min(len(issued) - 1 - pos, 15)
            if cnt is not None:
                waited_upto[0] = len(issued) - 1 - cnt
            if period == 1:
                if cnt is not None:
                    lines.append(f"s_waitcnt lgkmcnt({cnt})")
                lines.append(text)
            own, nxt = gap_items(g)
            for t in own:
                if t.kind in in_order:
                    issued.append((period, t.key))
                    issue_gap.append(period * NS + g)
                if period == 1:
                    lines.append(t.text)
            for t in nxt:
                if t.kind in in_order:
                    issued.append((period + 1, t.key))
                    issue_gap.append(period * NS + g)
                if period == 1:
                    lines.append("@N " + t.text)
    # prologue = the wrapped tasks alone, in the same order
    pro = []
    for g in range(NS):
        for t in per_gap.get(g - NS, []):
            pro.append("@N " + t.text)
    return lines, pro


def schedule(mfma, tasks, NS, budget=GAP_BUDGET, **waits):
    """place() + render_lines(): (body lines, prologue lines, per-gap load).  The tasks carry their gaps afterwards."""
    per_gap, load = place(tasks, NS, budget)
    return render_lines(mfma, per_gap, NS, **waits) + (load,)


class Once:
    """A resolve() hook: `what` goes in front of the first line for which when(index, line, is_next) holds."""

    def __init__(self, when, what=BARRIER):
        self.when, self.what, self.done = when, what, False

    def __call__(self, i, l, is_next):
        if self.done or not self.when(i, l, is_next):
            return []
        self.done = True
        return self.what


def resolve(lines, cur, nxt, split=True, rules=(), before=None):
    """Substitutes the placeholders of a rendered body.  '@KEY+n' becomes cur[KEY] + n, or nxt[KEY] + n in the lines tagged
    '@N ' (the next body's early work; the tag goes).  rules = (regex, function(match, is_next)) pairs for placeholders of
    another form, applied first.  before(index, line, is_next) returns the lines to insert in front of a line (barriers,
    waits) and may assert what it likes about the order of what it sees.  split: the instructions of a task become lines
    of their own (not those of an '@N ' task)."""
    if split:
        lines = [part for l in lines for part in (l.split("\n\t") if not l.startswith("@N ") else [l])]
    pat = "@(" + "|".join(cur) + r")\+(\d+)"
    out = []
    for i, l in enumerate(lines):
        is_next = l.startswith("@N ")
        if is_next:
            l = l[3:]
        b = nxt if is_next else cur
        if before:
            out.extend(before(i, l, is_next))
        for rx, fn in rules:
            l = re.sub(rx, lambda m: fn(m, is_next), l)
        out.append(re.sub(pat, lambda m: str(b[m.group(1)] + int(m.group(2))), l))
    return out


def c_string(lines):
    return " \\\n".join('    "' + l.replace("\n\t", "\\n\\t") + '\\n\\t"' for l in lines)


def define(name, lines):
    return f"#define {name} \\\n" + c_string(lines) + "\n"


def define_prologue(name, lines):
    """The early work of the very first body, as a statement of its own."""
    return define(name, lines + ["s_waitcnt lgkmcnt(0)"])      # in steady state the previous body's last waits cover these reads


def one_prologue(pros):
    """pros: the prologue lines of every variant of a body.  Variants follow each other in any order, so there is one."""
    assert len(set(map(tuple, pros))) == 1, "every body must leave the same reads in flight for the next one"
    return list(pros[0])


def file_text(chunks, check=False):
    """The text of a generator's .inc file; chunks(check) returns its pieces (or prints the --check report instead)."""
    return "\n".join(chunks(check))


def main(inc_name, chunks):
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "cuda_flashattention_amd", "csrc", inc_name))
    args = ap.parse_args()
    text = file_text(chunks, args.check)
    if not args.check:
        with open(args.out, "w") as f:
            f.write(text)
        print("wrote", args.out)
