#!/usr/bin/env python3
"""Compare the kernels of two device-assembly files (hipcc <CXXFLAGS> --offload-device-only -S): resource metadata, v_mfma
count, instructions between the first and the last v_mfma (the k-loop with its prologue tile) and whether the instruction
streams are identical after normalising symbol names and label numbers.  Prints one markdown table row per kernel;
--diff KERNEL_SUBSTRING prints the unified diff of the normalised streams of the kernels whose name contains it.

--rename REGEX=REPLACEMENT (repeatable) rewrites the kernel names of OLD.s before they are matched, for a change that drops a
template parameter: --rename 'gemm_split_pipe_kernel<(\d), 0, (\d)>=gemm_split_pipe_kernel<\1, \2>'.

    python tools/compare_kernel_isa.py OLD.s NEW.s [--diff SUBSTRING] [--rename REGEX=REPLACEMENT]...
"""
import difflib
import re
import subprocess
import sys

META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, out))


def short(name):
    """demangled kernel name without return type, namespaces and argument list"""
    name = re.sub(r"\((anonymous namespace|[a-z_0-9]+)\)::|gdrnpp::(splitgemm::|split2::)?", "", name)
    name = re.sub(r"^void ", "", name)
    return re.sub(r"\(.*$", "", name)


def parse(path):
    text = open(path).read()
    kernels = {}
    # bodies: "NAME:" ... "s_endpgm" of every symbol declared .amdhsa_kernel
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)", text, re.M):
        kernels[m.group(1)] = {}
    for name in kernels:
        start = text.index("\n%s:" % name)
        end = text.index(".Lfunc_end", start)
        body = []
        for line in text[start:end].split("\n")[2:]:
            line = re.sub(r"\s*;.*$", "", line).strip()
            if not line or line.startswith("."):
                if re.match(r"\.LBB\d+_\d+:", line):
                    body.append("LABEL:")
                continue
            line = re.sub(r"\.LBB\d+_(\d+)", "LBB", line)
            line = re.sub(r"_ZN?[A-Za-z0-9_]*zero_pageE?", "ZERO_PAGE", line)
            body.append(re.sub(r"\s+", " ", line))
        kernels[name]["body"] = body
        mf = [i for i, ins in enumerate(body) if ins.startswith("v_mfma")]
        kernels[name]["mfma"] = len(mf)
        kernels[name]["span"] = (mf[-1] - mf[0] + 1) if mf else 0
        kernels[name]["span_body"] = body[mf[0]:mf[-1] + 1] if mf else []
    # metadata: YAML note, one "- .agpr_count:" block per kernel with ".name:"
    for block in re.split(r"\n  - \.agpr_count:", text)[1:]:
        block = ".agpr_count:" + block
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        if name in kernels:
            for key in META:
                m = re.search(r"%s:\s+(\d+)" % re.escape(key), block)
                kernels[name][key] = int(m.group(1)) if m else None
    return kernels


def main():
    args = sys.argv[1:]
    want = None
    if "--diff" in args:
        i = args.index("--diff")
        want = args[i + 1]
        del args[i:i + 2]
    renames = []
    while "--rename" in args:
        i = args.index("--rename")
        renames.append(args[i + 1].split("=", 1))
        del args[i:i + 2]
    old, new = parse(args[0]), parse(args[1])
    names = demangle(sorted(set(old) | set(new)))
    by_short = lambda ks: {short(names[k]): v for k, v in ks.items()}
    old, new = by_short(old), by_short(new)
    for pat, repl in renames:
        old = {re.sub(pat, repl, k): v for k, v in old.items()}
    print("| kernel | vgpr | agpr | sgpr | spill | scratch | LDS | v_mfma | k-loop span | stream |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    ok = True
    for k in sorted(set(old) | set(new)):
        if k not in old or k not in new:
            print("| `%s` | only in %s |" % (k, "old" if k in old else "new"))
            ok = False
            continue
        a, b = old[k], new[k]
        cell = lambda key: str(a[key]) if a[key] == b[key] else "%s -> %s" % (a[key], b[key])
        same = a["body"] == b["body"]
        span_same = a["span_body"] == b["span_body"]
        verdict = "identical" if same else ("differs outside the span (%d -> %d instructions)" % (len(a["body"]), len(b["body"])) if span_same else "DIFFERS INSIDE THE SPAN")
        must = [".vgpr_count", ".agpr_count", ".vgpr_spill_count", ".private_segment_fixed_size", ".group_segment_fixed_size", "mfma", "span"]
        if not span_same or any(a[key] != b[key] for key in must):
            ok = False
        print("| `%s` | %s | %s | %s | %s | %s | %s | %s | %s | %s |" % (k, cell(".vgpr_count"), cell(".agpr_count"), cell(".sgpr_count"), cell(".vgpr_spill_count"),
                                                                       cell(".private_segment_fixed_size"), cell(".group_segment_fixed_size"), cell("mfma"), cell("span"), verdict))
        if want and want in k and not same:
            sys.stdout.write("\n".join(difflib.unified_diff(a["body"], b["body"], "old " + k, "new " + k, lineterm="", n=2)) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
