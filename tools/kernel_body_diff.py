"""Kernel-by-kernel comparison of the gfx950 code of one translation unit at two commits: which kernels kept their code.

usage: python tools/kernel_body_diff.py [--rev HEAD] [--unit vc_tokens] [--rename 'REGEX=>TEXT'] > profiles/<name>.log
--rename rewrites the PARENT's demangled kernel names first (re.sub), for a template that gained a defaulted parameter: with
--rename '(rows_attn_k<[^>]*)>=>\\1, false>' the parent's rows_attn_k<bf16_t, true, true, true> is held against <..., true, false>;
a 3-parameter name gets its defaulted 4th first (--rename may be given several times, applied in order).
Compiles voicecraft_amd/csrc/<unit>.hip device-only (hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S) from the
working tree and from `git show <rev>:` copies of csrc/ and include/ in a temporary directory, then compares each kernel's
instruction lines (up to the kernel's .Lfunc_end label) after dropping comments, directives and the function index inside basic-block
labels (.LBB<n>_)."""
import argparse, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_store_scan as isa  # noqa: E402


def compile_unit(tree, unit, out):
    src = os.path.join(tree, "voicecraft_amd", "csrc", unit + ".hip")
    r = subprocess.run([isa.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S", src, "-o", out],
                       cwd=os.path.dirname(src), stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    return open(out).read()


def checkout(rev, dst):
    for d in ("voicecraft_amd/csrc", "include"):
        os.makedirs(os.path.join(dst, d), exist_ok=True)
        names = subprocess.run(["git", "ls-tree", "--name-only", f"{rev}:{d}"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.split()
        for n in names:
            blob = subprocess.run(["git", "show", f"{rev}:{d}/{n}"], cwd=ROOT, capture_output=True, check=True).stdout
            open(os.path.join(dst, d, n), "wb").write(blob)


def instructions(body):
    # a kernel's code ends at its .Lfunc_end label (basic blocks may follow its last s_endpgm).  What isa.kernels() hands over runs
    # to the next kernel's head, and for the unit's LAST kernel to the end of the file: the compilation-unit id and the metadata table
    body = re.split(r"^\.Lfunc_end\d+:", body, maxsplit=1, flags=re.M)[0]
    out = []
    for line in body.splitlines():
        t = line.split(";")[0].strip()
        if not t or (t.startswith(".") and not t.startswith(".LBB")):
            continue
        out.append(re.sub(r"\.LBB\d+_", ".LBB_", t))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rev", default="HEAD")
    ap.add_argument("--unit", default="vc_tokens")
    ap.add_argument("--rename", action="append", default=[])
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        checkout(a.rev, os.path.join(tmp, "parent"))
        old = {isa.demangle(n): v for n, v in isa.kernels(compile_unit(os.path.join(tmp, "parent"), a.unit, os.path.join(tmp, "old.s"))).items()}
        new = {isa.demangle(n): v for n, v in isa.kernels(compile_unit(ROOT, a.unit, os.path.join(tmp, "new.s"))).items()}
    for r in a.rename:
        pat, rep = r.split("=>", 1)
        old = {re.sub(pat, rep, n): v for n, v in old.items()}
    print(f"# gfx950 disassembly of voicecraft_amd/csrc/{a.unit}.hip (hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S),")
    print("# parent commit against this build, kernel by kernel: instruction lines after dropping comments and directives and the")
    print("# function index inside basic-block labels (.LBB<n>_)")
    for name, (body, scratch, vgpr) in new.items():
        facts = f"scratch {scratch} bytes, next_free_vgpr {vgpr}, stores waiting for an earlier store: {isa.store_chains(body)[0]}"
        if name not in old:
            print(f"{name[:72]:72s} new kernel: {facts}")
            continue
        i0, i1 = instructions(old[name][0]), instructions(body)
        if i0 == i1:
            print(f"{name[:72]:72s} {len(i1):5d} lines  IDENTICAL")
        else:
            n_diff = sum(x != y for x, y in zip(i0, i1)) + abs(len(i0) - len(i1))
            print(f"{name[:72]:72s} CHANGED: {len(i0)} -> {len(i1)} lines, {n_diff} differ; {facts} (parent: scratch {old[name][1]}, "
                  f"next_free_vgpr {old[name][2]}, waiting stores {isa.store_chains(old[name][0])[0]})")
    for name in old:
        if name not in new:
            print(f"{name[:72]:72s} REMOVED")


if __name__ == "__main__":
    main()
