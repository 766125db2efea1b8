"""Instruction counts and resources per device function of pt_kernels.hip (code size matters: the shading kernels are
instruction-fetch bound; VGPRs, LDS and the private segment set occupancy and scratch traffic).
Usage: python tools/isa_stats.py [--part N] [--json FILE] [extra hipcc flags]
--part N compiles one MIPT_PART of the file as the Makefile does (0: every kernel but k_shade, 1-3 and 5: the k_shade instances in
four groups, 4: the BSDF probe's kernels); without it the whole file is one translation unit. --json FILE also writes {function: figures}.
The compile flags are the Makefile's (`make print-hipflags`: those of the part, or without --part the ones every unit shares);
extra flags come after them, so `-Xarch_device -fslp-vectorize` shows a part as plain -O3 makes it.
The report is about resources only: instruction classes are counted by prefix, no particular instruction is looked for."""
import collections, json, os, re, shutil, subprocess, sys, tempfile

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def makefile_flags(part):
    """The device compile flags of the Makefile (its print-hipflags target): those of unit part<N>, or without a part the
    flags every unit shares."""
    out = subprocess.check_output(["make", "-s", "--no-print-directory", "print-hipflags", "UNIT=" + ("" if part is None else "part%d" % part)],
                                  cwd=root, text=True)
    return out.split()


def compile_asm(flags, workdir, part=None):
    out = os.path.join(workdir, "pt_isa.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc"] + makefile_flags(part) +
                          ["--offload-device-only", "-S", "pbrt-v3-spectral_amd/csrc/device/pt_kernels.hip", "-o", out] + flags,
                          cwd=root, stderr=subprocess.DEVNULL)
    with open(out) as f:
        return f.read().split("\n")


def kernel_resources(lines):
    """{kernel symbol: {field: value}} from the code object's metadata (amdhsa.kernels): the final figures of each kernel."""
    res, cur = {}, None
    for l in lines:
        m = re.match(r"^(  - |    )\.(\w+):\s+(\S+)\s*$", l)
        if not m:
            continue
        if m.group(1) == "  - ":
            cur = {}
        if cur is None:
            continue
        cur[m.group(2)] = m.group(3)
        if m.group(2) == "name":
            res[m.group(3)] = cur
    return res


def short_name(n):
    return re.sub(r"N3dpt6DScene.*", "", n).replace("_ZN12_GLOBAL__N_1", "")


def stats(lines):
    starts = [(i, l.split(":")[0]) for i, l in enumerate(lines) if re.match(r"^[_A-Za-z0-9.$]+:\s+; @", l)]
    starts.append((len(lines), "end"))
    vg = dict(re.findall(r"\.set (\S+)\.num_vgpr, (\S.*)", "\n".join(lines)))
    res = kernel_resources(lines)
    rows = collections.OrderedDict()
    for (i, n), (j, _) in zip(starts, starts[1:]):
        c = collections.Counter()
        for l in lines[i:j]:
            if l.startswith(".Lfunc_end"):
                break
            m = re.match(r"\t([a-z_0-9]+)\s", l + " ")
            if m and not l.startswith("\t."):
                c[m.group(1)] += 1
        g = lambda p: sum(v for k, v in c.items() if k.startswith(p))
        r = res.get(n, {})
        field = lambda k: int(r[k]) if k in r else None
        rows[n] = {"insts": sum(c.values()), "gload": g(("global_load", "flat_load", "buffer_load")),
                   "gstore": g(("global_store", "flat_store", "buffer_store")), "scratch": g("scratch_"),
                   "f64": sum(v for k, v in c.items() if "f64" in k), "call": c["s_swappc_b64"],
                   "valu": g("v_"), "pk_f32": sum(v for k, v in c.items() if k.startswith("v_pk_") and k.endswith("_f32")),
                   "vmov": g("v_mov_"), "vgpr_spills": field("vgpr_spill_count"),
                   "vgpr": field("vgpr_count") if r else vg.get(n, "?")[:12], "private_bytes": field("private_segment_fixed_size"),
                   "lds_bytes": field("group_segment_fixed_size")}
    return rows


def main(argv):
    flags, part, json_file = [], None, None
    it = iter(argv)
    for a in it:
        if a == "--part":
            part = int(next(it))
        elif a == "--json":
            json_file = next(it)
        else:
            flags.append(a)
    if part is not None:
        flags.append("-DMIPT_PART=%d" % part)
    workdir = tempfile.mkdtemp(prefix="isa_stats_")
    try:
        rows = stats(compile_asm(flags, workdir, part))
    finally:
        shutil.rmtree(workdir, ignore_errors=True)
    show = lambda v: "-" if v is None else str(v)
    for n, r in rows.items():
        print("%-62s insts %6d valu %6d pk_f32 %4d vmov %4d gload %4d gstore %3d scratch %4d f64 %5d call %3d vgpr %s spills %s private %s lds %s" % (
            short_name(n)[:62], r["insts"], r["valu"], r["pk_f32"], r["vmov"], r["gload"], r["gstore"], r["scratch"], r["f64"], r["call"],
            show(r["vgpr"]), show(r["vgpr_spills"]), show(r["private_bytes"]), show(r["lds_bytes"])))
    if json_file:
        with open(json_file, "w") as f:
            json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
