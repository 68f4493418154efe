"""Does a refactor of csrc/ leave the compiled kernels alone?  Compiles every csrc/*.hip of two trees for the device with build()'s flags and compares,
per kernel symbol, (1) the compiler's resource report (-Rpass-analysis=kernel-resource-usage: SGPRs, VGPRs, AGPRs, scratch, occupancy, spills, LDS) and (2) the
instruction text (-S, comments and directives stripped, labels kept).  A kernel is `identical`, `reordered` (same number of instructions and the same opcode
histogram: operands or order moved, nothing added or removed) or `DIFFERENT`.  No GPU needed.
Kernels are paired by demangled name without the parameter list (`dce_grad_kernel<2>`), and the function index of a local label (`.LBB7_3`, `.Lfunc_end7`: the
function's place in the file, no instruction) is dropped, so a kernel that moved or whose parameter types were renamed still compares.  Where the refactor renames
kernels or adds template arguments, `--pair 'REGEX=REPLACEMENT'` (re.sub on the parent's names, repeatable) says which kernel became which.
usage: python scripts/codegen_diff.py <parent tree> <this tree> [file.hip ...] [--pair R=S ...]   exit status 1 if a resource column or a kernel's instructions differ"""
import collections, glob, os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import HIPCC_FLAGS


def kernel_names(symbols, pairs=()):
    """{symbol: demangled name, no namespace, return type or parameter list, after the --pair substitutions}"""
    # _Float16 (DF16_) as __fp16 (Dh), which binutils' c++filt knows: both are builtin types, and the parameter list is dropped below
    out = subprocess.run(["c++filt"], input="\n".join(symbols).replace("DF16_", "Dh"), capture_output=True, text=True, check=True).stdout.splitlines()
    names = {}
    for sym, d in zip(symbols, out):
        d = re.sub(r"^void ", "", d.replace("(anonymous namespace)::", "")).split("(")[0]
        for rx, to in pairs:
            d = re.sub(rx, to, d)
        names[sym] = d
    return names


def compile_one(src, tmp, pairs=()):
    """-> ({kernel: {column: value}}, {kernel: [instruction lines]}) of one source file"""
    out = os.path.join(tmp, os.path.basename(src) + ".s")
    r = subprocess.run([os.environ.get("HIPCC", "hipcc")] + HIPCC_FLAGS + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", src, "-o", out],
                       capture_output=True, text=True)
    if r.returncode:
        sys.exit(f"{src}: hipcc failed\n{r.stderr[-2000:]}")
    res, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: (?:.*: )?Function Name: (\S+)", line)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark: (?:\S+:\d+:\d+: )?([^:]+): (\S+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    text, sym = {}, None
    for line in open(out):
        line = line.split(";")[0].rstrip()
        m = re.match(r"([A-Za-z_][\w$.]*):$", line)
        if m:
            sym = m.group(1)
            text[sym] = []
        elif sym and line.strip() and (not line.lstrip().startswith(".") or line.endswith(":")):
            text[sym].append(re.sub(r"\.(LBB|Lfunc_end)\d+", r".\1", line.strip()))
    names = kernel_names(sorted(res), pairs)
    assert len(set(names.values())) == len(names), f"{src}: two kernels share a name after pairing"
    return {names[k]: v for k, v in res.items()}, {names[k]: v for k, v in text.items() if k in res}


def main():
    argv = sys.argv[1:]
    pairs = [tuple(argv[i + 1].split("=", 1)) for i, a in enumerate(argv) if a == "--pair"]
    argv = [a for i, a in enumerate(argv) if a != "--pair" and (i == 0 or argv[i - 1] != "--pair")]
    parent, change = argv[0], argv[1]
    only = set(argv[2:])
    names = sorted({os.path.basename(f) for t in (parent, change) for f in glob.glob(os.path.join(t, "ldiffusion_amd", "csrc", "*.hip"))})
    names = [n for n in names if not only or n in only]
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb, ThreadPoolExecutor(max_workers=8) as ex:
        jobs = {(n, i): ex.submit(compile_one, os.path.join(t, "ldiffusion_amd", "csrc", n), tmp, () if i else pairs)
                for n in names for i, (t, tmp) in enumerate(((parent, ta), (change, tb))) if os.path.exists(os.path.join(t, "ldiffusion_amd", "csrc", n))}
        got = {k: j.result() for k, j in jobs.items()}
    print("flags: hipcc " + " ".join(HIPCC_FLAGS) + " --cuda-device-only -S -Rpass-analysis=kernel-resource-usage")
    for rx, to in pairs:
        print(f"paired: parent's {rx} -> {to}")
    print("columns: file | kernels | resource report | identical text | reordered | DIFFERENT")
    bad, notes = 0, []
    for n in names:
        if (n, 0) not in got or (n, 1) not in got:
            print(f"{n} | only in the {'parent' if (n, 0) in got else 'change'}")
            bad += 1
            continue
        (ra, ta_), (rb, tb_) = got[(n, 0)], got[(n, 1)]
        kernels = sorted(set(ra) | set(rb))
        res_diff = [k for k in kernels if ra.get(k) != rb.get(k)]
        cls = collections.Counter()
        for k in kernels:
            a, b = ta_.get(k), tb_.get(k)
            same_ops = a is not None and b is not None and len(a) == len(b) and collections.Counter(l.split()[0] for l in a) == collections.Counter(l.split()[0] for l in b)
            c = "identical" if a == b and a is not None else "reordered" if same_ops else "DIFFERENT"
            cls[c] += 1
            if c == "reordered":
                notes.append(f"  reordered: {n} {k}: {len(a)} instructions, {sum(x != y for x, y in zip(a, b))} lines differ")
            if c == "DIFFERENT":
                notes.append(f"  DIFFERENT: {n} {k}: {len(a or [])} -> {len(b or [])} instructions")
        for k in res_diff:
            notes.append(f"  resources: {n} {k}: {ra.get(k)} -> {rb.get(k)}")
        bad += len(res_diff) + cls["DIFFERENT"]
        print(f"{n} | {len(kernels)} | {'equal' if not res_diff else str(len(res_diff)) + ' DIFFER'} | {cls['identical']} | {cls['reordered']} | {cls['DIFFERENT']}")
    print("\n".join(notes) if notes else "no kernel differs")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
