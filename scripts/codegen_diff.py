"""Does a refactor of csrc/ leave the compiled kernels alone?  Compiles every csrc/*.hip of two trees for the device with build()'s flags and compares,
per kernel symbol, (1) the compiler's resource report (-Rpass-analysis=kernel-resource-usage: SGPRs, VGPRs, AGPRs, scratch, occupancy, spills, LDS) and (2) the
instruction text (-S, comments and directives stripped, labels kept).  A kernel is `identical`, `reordered` (same number of instructions and the same opcode
histogram: operands or order moved, nothing added or removed) or `DIFFERENT`.  No GPU needed.
usage: python scripts/codegen_diff.py <parent tree> <this tree> [file.hip ...]      exit status 1 if a resource column or a kernel's instructions differ"""
import collections, glob, os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import HIPCC_FLAGS


def compile_one(src, tmp):
    """-> ({kernel: {column: value}}, {symbol: [instruction lines]}) of one source file"""
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
            text[sym].append(line.strip())
    return res, {k: v for k, v in text.items() if k in res}


def main():
    parent, change = sys.argv[1], sys.argv[2]
    only = set(sys.argv[3:])
    names = sorted({os.path.basename(f) for t in (parent, change) for f in glob.glob(os.path.join(t, "ldiffusion_amd", "csrc", "*.hip"))})
    names = [n for n in names if not only or n in only]
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb, ThreadPoolExecutor(max_workers=8) as ex:
        jobs = {(n, i): ex.submit(compile_one, os.path.join(t, "ldiffusion_amd", "csrc", n), tmp)
                for n in names for i, (t, tmp) in enumerate(((parent, ta), (change, tb))) if os.path.exists(os.path.join(t, "ldiffusion_amd", "csrc", n))}
        got = {k: j.result() for k, j in jobs.items()}
    print("flags: hipcc " + " ".join(HIPCC_FLAGS) + " --cuda-device-only -S -Rpass-analysis=kernel-resource-usage")
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
