"""gfx950 instruction streams of .hip files in two trees:  python tools/isa_diff.py <tree A> <tree B> mlp3.hip [mlp2.hip ...]
Each file is compiled with the library's flags plus --cuda-device-only -S; directive lines, comment lines and the per-build
__hip_cuid_* symbol are dropped.  Prints `identical`, or the number of differing lines and, for every kernel that differs, its
register / spill / LDS figures and MFMA count in both trees and the opcodes whose counts differ.
Where code moved between files:  python tools/isa_diff.py --by-kernel <tree A> a.hip [b.hip ...] -- <tree B> c.hip [d.hip ...]
pairs the kernels of the two file lists by mangled name (an anonymous-namespace kernel keeps its name whichever file holds it) and
compares each pair's ordered code lines without their trailing comments, block labels .LBB<function index>_<n> taken without the
index, which moves as soon as a file gains or loses a function.  Prints the kernels found on one side only, the table above for every
pair that differs, and the counts.  Where a move also renamed a type in the kernels' signatures (out of an anonymous namespace, say):
    python tools/isa_diff.py --by-kernel --rename OLD=NEW <tree A> ...
replaces OLD by NEW in the first tree's kernel names before pairing."""
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
    """{kernel: {metadata key: value, 'code': its code lines, comments and block labels' function index off, 'ops': Counter of its opcodes}}"""
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
        k["code"] = [re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", l.split(";")[0].rstrip()) for l in code_lines(lines[start + 1:end])]
        k["ops"] = Ops(l.split()[0] for l in k["code"] if not l.split()[0].endswith(":"))
    return meta


def table(names, ka, kb):
    for k in names:
        x, y = ka.get(k, {}), kb.get(k, {})
        ox, oy = x.get("ops", Ops()), y.get("ops", Ops())
        mfma = [sum(v for o, v in c.items() if o.startswith("v_mfma")) for c in (ox, oy)]
        rows = [(q, x.get(q, "-"), y.get(q, "-")) for q in KEYS] + [("instructions", sum(ox.values()), sum(oy.values())),
                                                                  ("v_mfma*", *mfma)]
        rows += [(o, ox[o], oy[o]) for o in sorted(set(ox) | set(oy)) if ox[o] != oy[o]]
        print(f"  {k}\n" + "\n".join(f"    {n:28s} {str(u):>8s} {str(w):>8s}" for n, u, w in rows))


def by_kernel(tree_a, names_a, tree_b, names_b, rename=None):
    with tempfile.TemporaryDirectory() as tmp:
        ka, kb = {}, {}
        for tree, names, into in ((tree_a, names_a, ka), (tree_b, names_b, kb)):
            for name in names:
                found = kernels(listing(tree, name, tmp))
                twice = sorted(set(found) & set(into))
                assert not twice, f"{name}: defined in another file of the same tree too: {twice}"
                into.update(found)
                print(f"{tree} {name}: {len(found)} kernels")
    if rename:
        ka = {k.replace(*rename): v for k, v in ka.items()}
    for side, only in (("first", sorted(set(ka) - set(kb))), ("second", sorted(set(kb) - set(ka)))):
        print(f"in the {side} tree only: {len(only)}" + "".join(f"\n  {k}" for k in only))
    both = sorted(set(ka) & set(kb))
    differ = [k for k in both if ka[k]["code"] != kb[k]["code"] or any(ka[k].get(q) != kb[k].get(q) for q in KEYS)]
    table(differ, ka, kb)
    print(f"{len(both)} kernels in both trees: {len(both) - len(differ)} identical ({sum(len(ka[k]['code']) for k in both)} lines), "
          f"{len(differ)} differ")


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
            table([k for k in sorted(set(ka) | set(kb)) if ka.get(k, {}).get("ops", Ops()) != kb.get(k, {}).get("ops", Ops())
                   or any(ka.get(k, {}).get(q) != kb.get(k, {}).get(q) for q in KEYS)], ka, kb)


if __name__ == "__main__":
    if sys.argv[1] == "--by-kernel":
        rename = sys.argv[3].split("=", 1) if sys.argv[2] == "--rename" else None
        args = sys.argv[4 if rename else 2:]
        cut = args.index("--")
        by_kernel(args[0], args[1:cut], args[cut + 1], args[cut + 2:], rename)
    else:
        main(sys.argv[1], sys.argv[2], sys.argv[3:])
