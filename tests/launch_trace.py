"""Which kernels did a call launch?  `launches()` records the library calls of its body as a launch plan (csrc/plan.cc: every
dg::launch is executed as usual AND appended to the plan), reads every kernel node back with dgcnn_plan_kernel and destroys the
plan.  The k-NN kernel forms return the same bits by design, and so do the GEMM tiles within one arithmetic: only the recorded
name tells a test whether the form it means to exercise is the one that ran.

parse_kernel_name() is pure Python (tests/test_launch_names.py pins it on the CPU); launches() needs the library and a GPU.

Not for use around a trainval step that itself runs in plan mode: there is one recorder per process and dgcnn_plan_begin
refuses a second."""
import contextlib
import re


ANON = "(anonymous namespace)::"


def _depth_scan(s):
    """Yield (i, ch, depth before ch) with depth counted over <...>, (...) and [...]."""
    depth = 0
    for i, ch in enumerate(s):
        if ch in ">)]":
            depth -= 1
        yield i, ch, depth
        if ch in "<([":
            depth += 1


def _split_top(s):
    """Split at the commas outside every bracket."""
    out, last = [], 0
    for i, ch, depth in _depth_scan(s):
        if ch == "," and depth == 0:
            out.append(s[last:i])
            last = i + 1
    out.append(s[last:])
    return [a.strip() for a in out]


def _open_of_last(s, close, open_):
    """Index of the bracket that opens the group closing at the end of s, or -1."""
    depth = 0
    for i in range(len(s) - 1, -1, -1):
        if s[i] == close:
            depth += 1
        elif s[i] == open_:
            depth -= 1
            if depth == 0:
                return i
    return -1


def _strip_scope(s):
    """`a::b::name<x::T, 3>` -> `name<T, 3>`: namespaces go at every level, brackets stay."""
    s = s.strip()
    cut = 0
    for i, ch, depth in _depth_scan(s):
        if depth == 0 and s.startswith("::", i):
            cut = i + 2
    s = s[cut:]
    if s.endswith(">"):
        lt = _open_of_last(s, ">", "<")
        if lt > 0:
            return s[:lt] + "<" + ", ".join(_clean_arg(a) for a in _split_top(s[lt + 1:-1])) + ">"
    return s


def _clean_arg(a):
    m = re.match(r"^\(([A-Za-z_ ]+)\)\s*(-?\w+)$", a.strip())            # "(bool)1", "(int)-3", "(unsigned int)4"
    if m:
        if m.group(1).strip() == "bool" and m.group(2) in ("0", "1"):
            return "true" if m.group(2) == "1" else "false"
        return m.group(2)
    return _strip_scope(a)


def parse_kernel_name(s):
    """'void (anonymous namespace)::knn_kernel<4, 20, (anonymous namespace)::PackedClouds>(float const*, ...)'
    -> ('knn_kernel', ['4', '20', 'PackedClouds']).  The return type, the namespaces and the parameter list go; template arguments
    are split at the top level only, so a nested template stays one argument (its own namespaces stripped); a cast such as
    '(bool)1' becomes 'true'.  A name without <...> gives an empty list; a string that is no demangled name (a raw mangled symbol)
    comes back as (s, [])."""
    t = s.strip().replace(ANON, "")
    if not t or t.startswith("_Z") or t.startswith("__Z"):
        return (s, [])
    if t.endswith(")"):                                                  # the parameter list
        lp = _open_of_last(t, ")", "(")
        if lp <= 0:
            return (s, [])
        t = t[:lp].rstrip()
    cut = 0
    for i, ch, depth in _depth_scan(t):                                  # the return type: up to the last top-level blank
        if ch == " " and depth == 0:
            cut = i + 1
    t = t[cut:]
    args = []
    if t.endswith(">"):
        lt = _open_of_last(t, ">", "<")
        if lt <= 0:
            return (s, [])
        args = [_clean_arg(a) for a in _split_top(t[lt + 1:-1])]
        t = t[:lt]
    base = _strip_scope(t)
    if not re.match(r"^[A-Za-z_]\w*$", base):
        return (s, [])
    return (base, args)


@contextlib.contextmanager
def launches():
    """with launches() as L: <library calls>  ->  afterwards L == [(base_name, template_args, grid, block, lds_bytes), ...], one
    tuple per kernel the body launched, in launch order (grid and block as (x, y, z)).  The calls execute normally.  A body that
    raises (refused calls raise ValueError) aborts the recording and leaves L empty."""
    from dgcnn import _hip as H
    out = []
    rec = H.Plan.record()
    plan = rec.__enter__()
    try:
        yield out
    except BaseException as e:
        rec.__exit__(type(e), e, e.__traceback__)            # dgcnn_plan_abort
        raise
    rec.__exit__(None, None, None)                           # dgcnn_plan_end
    try:
        for name, g, b, lds in plan.kernels():
            base, args = parse_kernel_name(name)
            out.append((base, args, g, b, lds))
    finally:
        plan.destroy()


def names(L):
    """The base names of a recorded list, in order."""
    return [e[0] for e in L]


def find(L, base, args=None):
    """The recorded launches of kernel `base` whose leading template arguments equal `args` (a '*' matches anything)."""
    hit = []
    for e in L:
        if e[0] != base:
            continue
        if args is not None:
            a = [str(x) for x in args]
            if len(e[1]) < len(a) or any(x != "*" and x != y for x, y in zip(a, e[1])):
                continue
        hit.append(e)
    return hit


def assert_launched(L, base, args=None):
    """`expect=` of the forced-form tests: kernel `base` (with these leading template arguments) is among those launched."""
    assert find(L, base, args), "expected %s%s among the launched kernels, recorded: %s" % (
        base, "" if args is None else "<%s>" % ", ".join(str(a) for a in args), [(e[0], e[1]) for e in L])


@contextlib.contextmanager
def timed():
    """A timer for the calls of the body; -> its records (the tag of a call is records[i][0])."""
    from dgcnn import _hip as H
    prev = H.TIMER
    H.TIMER = tm = H.Timer()
    try:
        yield tm.records
    finally:
        H.TIMER = prev


def check_kernels(L, expect, what):
    got = [(e[0], e[1]) for e in L]
    assert [g[0] for g in got] == [e[0] for e in expect], "%s: launched %s, expected %s" % (what, got, expect)
    for (name, args), (_, want) in zip(got, expect):
        assert len(args) >= len(want) and all(w == "*" or w == a for w, a in zip(want, args)), \
            "%s: %s<%s> launched, expected <%s>" % (what, name, ", ".join(args), ", ".join(want))
