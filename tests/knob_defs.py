"""The environment knobs as the library defines them: g_knobs in utmos_amd/csrc/utmos_hip.hip (name, default, legal
range), read as text.  Needs no GPU and no build: the knob tests take their sweep values from here, and the CPU test
(test_knob_table.py) checks the header's Environment list and the sweep table against it."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "utmos_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "utmos_hip.h")
INT_MAX = 2 ** 31 - 1

_KNOB_RE = re.compile(r'UTM_KNOB_(I|D|STEP|SET)\("(\w+)", (\w+), ([^)]*?)\),')


def _constants():
    """#define / constexpr integer constants of the csrc headers the knob table may name (UTM_LOOP_MAX_LOCAL, ...)."""
    text = ""
    for f in sorted(os.listdir(CSRC)):
        if f.endswith(".h") or f.endswith(".hip"):
            text += open(os.path.join(CSRC, f)).read() + "\n"
    defs = dict(re.findall(r"^#define (UTM_\w+) (\(?[0-9][^/\n]*?)\s*(?://.*)?$", text, re.M))
    for name, expr in re.findall(r"constexpr unsigned (UTM_\w+) = ([^;]+);", text):
        defs[name] = expr
    return defs


def _eval(expr, defs, depth=0):
    expr = expr.strip()
    if expr == "INT_MAX":
        return INT_MAX
    for name in sorted(set(re.findall(r"\bUTM_\w+\b", expr)), key=len, reverse=True):
        assert depth < 8 and name in defs, (name, expr)
        expr = re.sub(r"\b%s\b" % name, "(%s)" % _eval(defs[name], defs, depth + 1), expr)
    expr = re.sub(r"(?<=[0-9])(ull|ul|u|ll)\b", "", expr)
    expr = re.sub(r"(.+?)\?(.+?):(.+)", r"(\2) if (\1) else (\3)", expr.replace("\n", " "))
    return eval(expr, {"__builtins__": {}})


_KNOBS = None


def knobs():
    """{name: dict(kind, field, default, lo, hi, step, set)} in table order; kind 'D' = float64, else int."""
    global _KNOBS
    if _KNOBS is not None:
        return _KNOBS
    src = open(os.path.join(CSRC, "utmos_hip.hip")).read()
    defs = _constants()
    out = {}
    for kind, name, field, rest in _KNOB_RE.findall(src):
        args = [a.strip() for a in rest.split(",")]  # (a set is one blank-separated string)
        k = {"kind": kind, "field": field, "default": _eval(args[0], defs), "lo": None, "hi": None, "step": 1, "set": None}
        if kind == "SET":
            k["set"] = [int(x) for x in args[1].strip('"').split()]
            k["lo"], k["hi"] = min(k["set"]), max(k["set"])
        else:
            k["lo"], k["hi"] = _eval(args[1], defs), _eval(args[2], defs)
            if kind == "STEP":
                k["step"] = _eval(args[3], defs)
        if kind == "D":
            k["default"], k["lo"], k["hi"] = float(k["default"]), float(k["lo"]), float(k["hi"])
        out[name] = k
    _KNOBS = out
    return out


def fmt(v):
    """A number as the header writes it: 2^k above 65,536, INT_MAX, %g for float64 knobs."""
    if isinstance(v, float):
        return "%g" % v
    if v == INT_MAX:
        return "INT_MAX"
    if v > 65536 and v & (v - 1) == 0:
        return "2^%d" % (v.bit_length() - 1)
    return str(v)


def range_text(k):
    if k["set"] is not None:
        return "{" + ", ".join(str(x) for x in k["set"]) + "}"
    text = "%s..%s" % (fmt(k["lo"]), fmt(k["hi"]))
    return text + (" step %d" % k["step"] if k["step"] != 1 else "")


def legal(k, v):
    if k["set"] is not None:
        return v in k["set"]
    return k["lo"] <= v <= k["hi"] and (k["kind"] == "D" or v % k["step"] == 0)


def sweep_values(k):
    """The default, both ends of the range, one legal value in between and one illegal value (as environment text)."""
    if k["set"] is not None:
        s = k["set"]
        mid = s[len(s) // 2]
        bad = next(x for x in range(s[0] + 1, s[-1] + 2) if x not in s)
    elif k["kind"] == "D":
        mid = (k["lo"] + k["hi"]) / 4
        bad = k["hi"] * 2 + 1
    else:
        step = k["step"]
        mid = (k["lo"] + k["hi"]) // 2 // step * step
        bad = k["hi"] + step if k["hi"] < INT_MAX else k["lo"] - 1
    vals = [k["default"], k["lo"], k["hi"], mid]
    out = []
    for v in vals:
        t = fmt_env(v)
        if t not in out:
            out.append(t)
    assert all(legal(k, type(k["default"])(float(v))) for v in out) and not legal(k, bad)
    return out, fmt_env(bad)


def fmt_env(v):
    return repr(float(v)) if isinstance(v, float) else str(int(v))


def header_entries():
    """{name: (default text, range text)} from the Environment list of include/utmos_hip.h: `NAME (default; range)`."""
    text = open(HEADER).read()
    env = text[text.index(" * Environment."):]
    env = env[:env.index(" */")]
    return {m[0]: (m[1].strip(), m[2].strip()) for m in re.findall(r"\b(UTM_[A-Z0-9_]+) \(([^;()]+); ([^()]+)\)", env)}
