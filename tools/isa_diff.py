"""gfx950 instruction streams of .hip files in two trees:  python tools/isa_diff.py <tree A> <tree B> mlp3.hip [mlp2.hip ...]
Each file is compiled with the library's flags plus --cuda-device-only -S; directive lines, comment lines and the per-build
__hip_cuid_* symbol are dropped.  Prints `identical`, or the number of differing lines and, for every kernel that differs, its
register / spill / LDS figures and MFMA count in both trees and the opcodes whose counts differ."""
import collections, difflib, os, re, subprocess, sys, tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import HIPCC_FLAGS

KEYS = ["vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
        "group_segment_fixed_size"]
Ops = collections.Counter


def listing(tree, name, tmp):
    out = os.path.join(tmp, f"{abs(hash(tree))}_{name}.s")
    flags = [f for f in HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + ["--cuda-device-only", "-S", name, "-o", out],
                   check=True, cwd=os.path.join(tree, "aur_ppo_amd", "csrc"))
    return open(out).read().splitlines()


def code_lines(lines):
    return [l for l in lines if not re.match(r"\s*(- )?\.(?!L)", l) and not l.lstrip().startswith(";") and "__hip_cuid_" not in l
            and l.strip()]


def kernels(lines):
    """{kernel: {metadata key: value, 'ops': Counter of its opcodes}}"""
    meta, cur = {}, None
    for l in lines:
        if re.match(r"  - \.", l):
            cur = {}
        m = re.match(r"  (?:- |  )\.(\w+):\s+(\S+)", l)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
            if m.group(1) == "name":
                meta[m.group(2)] = cur
    for name, k in meta.items():
        start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        k["ops"] = Ops(l.split()[0] for l in code_lines(lines[start + 1:end]) if not l.split()[0].endswith(":"))
    return meta


def main(tree_a, tree_b, names):
    with tempfile.TemporaryDirectory() as tmp:
        for name in names:
            a, b = listing(tree_a, name, tmp), listing(tree_b, name, tmp)
            ca, cb = code_lines(a), code_lines(b)
            if ca == cb:
                print(f"{name}: identical ({len(ca)} lines)")
                continue
            n = sum(1 for d in difflib.ndiff(ca, cb) if d[:2] in ("- ", "+ "))
            print(f"{name}: {n} differing lines")
            ka, kb = kernels(a), kernels(b)
            for k in sorted(set(ka) | set(kb)):
                x, y = ka.get(k, {}), kb.get(k, {})
                ox, oy = x.get("ops", Ops()), y.get("ops", Ops())
                if ox == oy and all(x.get(q) == y.get(q) for q in KEYS):
                    continue
                mfma = [sum(v for o, v in c.items() if o.startswith("v_mfma")) for c in (ox, oy)]
                rows = [(q, x.get(q, "-"), y.get(q, "-")) for q in KEYS] + [("instructions", sum(ox.values()), sum(oy.values())),
                                                                          ("v_mfma*", *mfma)]
                rows += [(o, ox[o], oy[o]) for o in sorted(set(ox) | set(oy)) if ox[o] != oy[o]]
                print(f"  {k}\n" + "\n".join(f"    {n:28s} {str(u):>8s} {str(w):>8s}" for n, u, w in rows))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], sys.argv[3:])
