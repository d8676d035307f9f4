"""Whether two hipcc -S listings (`make isa`) hold the same device code,
function by function: every function of listing A must be in listing B with
the same instructions.  Local labels (.LBB<n>_<m>, .Lfunc_end<n>, ...) are
numbered per function in the order of the translation unit, so a function
added before another renumbers the latter's labels: the function number is
taken out of them before comparing, nothing else.

    python scripts/isa_same.py PARENT.s THIS.s

Prints the functions of A that are missing from B or differ, and those B adds;
exit status 1 when a function of A is missing or differs.
"""
import re
import sys


def functions(text):
    """{symbol: [instruction lines]} of every function body in the listing."""
    out = {}
    for m in re.finditer(r"^([\w.$]+):[ \t]*(?:;[^\n]*)?\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        body = []
        for line in m.group(2).splitlines():
            line = line.split(";")[0].rstrip()
            if not line or line.lstrip().startswith((".p2align", ".loc", ".file", ".cfi")):
                continue
            body.append(re.sub(r"\.L(BB|func_begin|func_end|tmp)\d+", r".L\1", line))
        out[m.group(1)] = body
    return out


def main():
    a, b = (functions(open(p).read()) for p in sys.argv[1:3])
    bad = 0
    for sym, body in a.items():
        if sym not in b:
            print("missing:", sym)
            bad += 1
        elif b[sym] != body:
            print(f"differs: {sym} ({len(body)} against {len(b[sym])} lines)")
            bad += 1
    for sym in b:
        if sym not in a:
            print("added:", sym)
    print(f"{len(a)} functions in {sys.argv[1]}, {len(b)} in {sys.argv[2]}, {bad} missing or different")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
