#!/usr/bin/env python3
"""Compares the gfx950 code of kernel sources (by default K1, K4 and K7) between two source trees, without a GPU.

Both trees' kernels/k1_fft_bank.hip, k4_demod.hip and k7_subtract.hip (or the files named with --sources) are compiled
to assembly with build.sh's FLAGS (plus --cuda-device-only -S), once plain and once with -DWSPR_LAB.  For every function symbol the opcode histogram
(mnemonic -> count) and, for kernels, the code-object metadata (vgpr_count, sgpr_count, group_segment_fixed_size,
private_segment_fixed_size, vgpr_spill_count) are compared.  Register numbers and the order of commutative operands are
not looked at: a refactor that leaves the arithmetic alone leaves both alone.

  python tools/kernel_isa_diff.py BASE_TREE NEW_TREE [--out profiles/arith_policy_isa.txt]
  python tools/kernel_isa_diff.py BASE_TREE NEW_TREE --sources k8_synth k13_fade k17_audio_synth k18_iq_audio
  (BASE_TREE: e.g. `git worktree add /tmp/parent HEAD~1`)
"""
import argparse
import collections
import concurrent.futures
import os
import re
import shutil
import subprocess
import sys
import tempfile

SOURCES = ("k1_fft_bank", "k4_demod", "k7_subtract")
META = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count")
# the exact instantiations of the kernels that each take >= 5 % of a configs[2] step (profiles/contracted_ab.txt)
GATED = ("sub_fir_fused_kernel<false>", "demod_lagsys_kernel<false>", "freq_scalar_kernel<false>",
         "demod_drift_kernel<false, false>", "freq_drift_kernel<false>")
# instantiations that a refactor renamed (base tree's name -> new tree's): compared with each other, under the new name
RENAMED = {
    "demod_drift_kernel<false>": "demod_drift_kernel<false, false>",
    "demod_drift_kernel<true>": "demod_drift_kernel<true, false>",
    "demod_drift_list_kernel<false>": "demod_drift_kernel<false, true>",
    "demod_drift_list_kernel<true>": "demod_drift_kernel<true, true>",
    "lag_exact_kernel<false>": "lag_exact_kernel<false, false>",
    "lag_exact_kernel<true>": "lag_exact_kernel<true, false>",
    "lag_exact_drift_kernel<false>": "lag_exact_kernel<false, true>",
    "lag_exact_drift_kernel<true>": "lag_exact_kernel<true, true>",
}


def build_flags(tree):
    sh = open(os.path.join(tree, "rtlsdr-wsprd_amd", "csrc", "build.sh")).read()
    flags = re.search(r'^FLAGS="(.*?)"', sh, re.M).group(1)
    return re.sub(r"\$\{[^}]*\}", "", flags).split()


def assembly(tree, src, extra):
    csrc = os.path.join(tree, "rtlsdr-wsprd_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, src + ".s")
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + build_flags(tree) + extra +
                       ["--cuda-device-only", "-S", "-Wno-unused-command-line-argument", "-x", "hip", os.path.join(csrc, "kernels", src + ".hip"), "-o", out],
                       check=True)
        return open(out).read()


def demangle(names):
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not names or not filt:
        return {n: n for n in names}
    out = subprocess.run([filt] + list(names), check=True, capture_output=True, text=True).stdout.split("\n")
    short = lambda s: re.sub(r"\(anonymous namespace\)::|wspr::|^void ", "", s).split("(")[0]
    return {n: short(o) for n, o in zip(names, out)}


def functions(asm):
    """symbol -> {"ops": Counter of mnemonics, "meta": {key: value} (kernels only)}."""
    funcs, cur = {}, None
    for line in asm.split("\n"):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = funcs.setdefault(m.group(1), {"ops": collections.Counter(), "meta": {}})
        elif re.match(r"^\.Lfunc_end\d+:", line):
            cur = None
        elif cur is not None and re.match(r"^\t[a-z]", line):
            cur["ops"][line.split()[0]] += 1
    for entry in re.split(r"\n  - ", asm[asm.find("amdhsa.kernels:"):])[1:]:
        kv = dict(re.findall(r"^ {0,4}\.(\w+):\s+(\S+)", "    " + entry, re.M))
        if kv.get("name") in funcs:
            funcs[kv["name"]]["meta"] = {k: kv.get(k, "0") for k in META}
    funcs = {k: v for k, v in funcs.items() if v["ops"]}          # (data symbols have no instructions)
    names = demangle(sorted(funcs))
    return {names[k]: v for k, v in funcs.items()}


def compare(base, new):
    """list of (function, [difference lines]) for every function that differs or exists on one side only."""
    out = []
    for name in sorted(set(base) | set(new)):
        if name not in base or name not in new:
            out.append((name, ["only in the %s tree" % ("new" if name in new else "base")]))
            continue
        b, n, lines = base[name], new[name], []
        for k in META:
            if b["meta"].get(k) != n["meta"].get(k):
                lines.append("%s: %s -> %s" % (k, b["meta"].get(k), n["meta"].get(k)))
        for op in sorted(set(b["ops"]) | set(n["ops"])):
            if b["ops"][op] != n["ops"][op]:
                lines.append("%s: %d -> %d" % (op, b["ops"][op], n["ops"][op]))
        if lines:
            out.append((name, lines))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("base")
    ap.add_argument("new")
    ap.add_argument("--out", default=None)
    ap.add_argument("--sources", nargs="+", default=list(SOURCES), metavar="NAME",
                    help="files of csrc/kernels/ without .hip (default: %s)" % " ".join(SOURCES))
    a = ap.parse_args()
    rep, gate_failed, gated_seen = [], False, set()
    variants = (("plain", []), ("-DWSPR_LAB", ["-DWSPR_LAB"]))
    jobs = [(tree, src, v) for v in range(2) for src in a.sources for tree in (a.base, a.new)]
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(6, os.cpu_count() or 1)) as pool:
        asm = dict(zip(jobs, pool.map(lambda j: functions(assembly(j[0], j[1], variants[j[2]][1])), jobs)))
    for v, (variant, extra) in enumerate(variants):
        for src in a.sources:
            base, new = asm[(a.base, src, v)], asm[(a.new, src, v)]
            base = {(RENAMED[k] if RENAMED.get(k) in new else k): f for k, f in base.items()}
            diffs = compare(base, new)
            rep.append("%s, %s.hip: %d functions in the base tree, %d in the new one, %d differ" % (
                variant, src, len(base), len(new), len(diffs)))
            for g in GATED:
                if g in new:
                    same = g in base and not any(name == g for name, _ in diffs)
                    gate_failed |= not same
                    gated_seen.add(g)
                    rep.append("  gated %-30s %s  (vgpr %s, sgpr %s, lds %s, scratch %s, spills %s; %d instructions)" % (
                        g, "identical" if same else "DIFFERS", *[new[g]["meta"].get(k) for k in META], sum(new[g]["ops"].values())))
            for name, lines in diffs:
                rep.append("  %s" % name)
                if name in new and new[name]["meta"]:          # a kernel: its resources in the new tree, changed or not
                    rep.append("      (new tree: vgpr %s, sgpr %s, lds %s, scratch %s, spills %s; %d instructions)" % (
                        *[new[name]["meta"].get(k) for k in META], sum(new[name]["ops"].values())))
                rep.extend("      " + l for l in lines)
    rep.append("")
    rep.append("GATE: " + ("FAILED -- a gated kernel differs" if gate_failed else
                           "none of the gated kernels is in these sources" if not gated_seen else
                           "passed -- the %s gated kernels are identical in opcode counts and resources in both builds"
                           % {5: "five"}.get(len(gated_seen), len(gated_seen))))
    text = "\n".join(rep) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    sys.stdout.write(text)
    return 1 if gate_failed else 0


if __name__ == "__main__":
    sys.exit(main())
