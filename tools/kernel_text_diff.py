#!/usr/bin/env python3
"""Compare the gfx950 device code of csrc/*.hip files between two source trees, on the CPU.

Every file is compiled on each side with build.py's flags plus --cuda-device-only -S and any -D given here; the lines that
hold a __hip_cuid symbol (a hash of the compile's inputs) are dropped and the two texts compared whole.  Per file: `equal`,
`reordered` (the same kernels with the same instructions, emitted in another order: host code decides the order in which
templates are instantiated) or `differs`, and for every kernel symbol of each side the numbers the assembler writes into the
code object's metadata.

    tools/kernel_text_diff.py                        # HEAD against the working tree, the files that include conv_common.h
    tools/kernel_text_diff.py -DFW_PAIR_STAMP conv3x3_pair.hip conv3x3_pair_slide.hip
    tools/kernel_text_diff.py --a /some/tree --b /other/tree -DFW_WRING=5

`--a` / `--b` take a directory or a git revision (exported with `git archive` into a temporary directory); `--b` defaults to
the working tree.  The result of a run is merged into --out under its label ("product" or the -D list)."""
from __future__ import annotations

import argparse
import json
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from framewright_amd import build as B  # noqa: E402

PKG = B.PKG_DIR.relative_to(ROOT)
CONV_COMMON_FILES = ["conv3x3_mfma.hip", "conv3x3_pair.hip", "conv3x3_pair_slide.hip", "conv3x3_pair_slide32.hip", "conv3x3_wino.hip",
                     "conv_up2x_phase.hip", "pointwise_gemm.hip", "pw_dw_fused.hip", "naf_tail128.hip"]
# the kernel descriptors of the code object's metadata (.amdgpu_metadata, one YAML map per kernel)
FIELDS = {"vgpr": ".vgpr_count", "sgpr": ".sgpr_count", "vgpr_spill": ".vgpr_spill_count", "sgpr_spill": ".sgpr_spill_count",
          "lds_bytes": ".group_segment_fixed_size", "scratch_bytes": ".private_segment_fixed_size"}


def export(spec: str, tmp: Path) -> Path:
    """A directory as it is; anything else is a git revision of this repository."""
    if Path(spec).is_dir():
        return Path(spec).resolve()
    dst = tmp / re.sub(r"\W", "_", spec)
    dst.mkdir()
    tar = subprocess.run(["git", "-C", str(ROOT), "archive", spec, str(PKG / "csrc"), "include"], check=True, capture_output=True).stdout
    subprocess.run(["tar", "-x", "-C", str(dst)], input=tar, check=True)
    return dst


def compile_text(tree: Path, name: str, defines: list[str], out: Path) -> str | None:
    """The device assembly of tree's csrc/name without its __hip_cuid lines; None where it does not compile."""
    csrc = tree / PKG / "csrc"
    cmd = [B.hipcc(), *B.CXXFLAGS, *B.PER_FILE_FLAGS.get(name, []), *defines, f"-I{tree / 'include'}", f"-I{csrc}",
           "--cuda-device-only", "-S", str(csrc / name), "-o", str(out)]
    if subprocess.run(cmd, capture_output=True, text=True).returncode != 0:
        return None
    return "".join(ln for ln in out.read_text().splitlines(keepends=True) if "__hip_cuid" not in ln)


def kernels(text: str) -> dict[str, dict[str, int]]:
    res: dict[str, dict[str, int]] = {}
    meta = text.split(".amdgpu_metadata", 1)[1] if ".amdgpu_metadata" in text else ""
    for block in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"^\s*\.name:\s*(\S+)", block, re.M)
        if name:
            res[name.group(1)] = {k: int(re.search(rf"^\s*{re.escape(f)}:\s*(\d+)", block, re.M).group(1)) for k, f in FIELDS.items()}
    for name, size in re.findall(r"^\s*\.size\s+(\S+), \.Lfunc_end\d+-\S+\n\s*; -- End function\n(?:.*\n)*?; codeLenInByte = (\d+)", text, re.M):
        if name in res:
            res[name]["code_bytes"] = int(size)
    return res


def bodies(text: str) -> dict[str, str]:
    """Every function's instructions by symbol, its labels freed of the function's position in the file."""
    res = {}
    for m in re.finditer(r"^(\S+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S):
        body = re.sub(r"(BB|func_begin|func_end|tmp)\d+", r"\1", m.group(2))   # labels, and the comments that quote them
        res[m.group(1)] = re.sub(r"[ \t]+;", " ;", body)
    return res


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--a", default="HEAD", help="first side: directory or git revision (default HEAD)")
    ap.add_argument("--b", default=str(ROOT), help="second side: directory or git revision (default: the working tree)")
    ap.add_argument("-D", dest="defines", action="append", default=[], metavar="NAME[=VALUE]")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "conv_common_isa.json"))
    ap.add_argument("--keep", metavar="DIR", help="leave the compared texts there as a_<file>.s and b_<file>.s, for diff")
    ap.add_argument("-j", type=int, default=16, help="parallel compiles (at most 16)")
    ap.add_argument("files", nargs="*", default=CONV_COMMON_FILES, help="names under csrc/ (default: the files that include conv_common.h)")
    args = ap.parse_args()
    defines = [f"-D{d}" for d in args.defines]
    label = " ".join(defines) or "product"
    with tempfile.TemporaryDirectory() as td:
        tmp = Path(td)
        trees = {"a": export(args.a, tmp), "b": export(args.b, tmp)}
        jobs = [(side, name) for name in args.files for side in ("a", "b")]
        with ThreadPoolExecutor(max_workers=max(1, min(16, args.j))) as ex:
            texts = dict(zip(jobs, ex.map(lambda j: compile_text(trees[j[0]], j[1], defines, tmp / f"{j[0]}_{j[1]}.s"), jobs)))
    result, bad = {}, 0
    for name in args.files:
        ta, tb = texts["a", name], texts["b", name]
        if ta is None and tb is None:
            verdict = "compiles on neither side"
        elif ta is None or tb is None:
            verdict = "compiles on one side only: " + ("b" if ta is None else "a")
        else:
            verdict = "equal" if ta == tb else ("reordered" if bodies(ta) == bodies(tb) and kernels(ta) == kernels(tb) else "differs")
        bad += verdict not in ("equal", "reordered", "compiles on neither side")
        if args.keep:
            Path(args.keep).mkdir(parents=True, exist_ok=True)
            for side, text in (("a", ta), ("b", tb)):
                (Path(args.keep) / f"{side}_{name}.s").write_text(text or "")
        a, b = kernels(ta or ""), kernels(tb or "")
        result[name] = {"text": verdict, "kernels": a} if a == b else {"text": verdict, "kernels_a": a, "kernels_b": b}
        print(f"{label}: {name}: {verdict}")
        for sym in sorted(set(a) | set(b)):
            ka, kb = a.get(sym), b.get(sym)
            if ka == kb:
                print(f"    {sym}: " + " ".join(f"{k}={v}" for k, v in ka.items()))
            else:
                print(f"    {sym}:\n        a: {ka}\n        b: {kb}")
    out = Path(args.out)
    record = json.loads(out.read_text()) if out.exists() else {}
    def name(spec: str) -> str:  # a revision by its hash: HEAD moves
        if Path(spec).is_dir():
            return "working tree" if Path(spec).resolve() == ROOT else spec
        return subprocess.run(["git", "-C", str(ROOT), "rev-parse", spec], check=True, capture_output=True, text=True).stdout.strip()

    record[label] = {"a": name(args.a), "b": name(args.b), "flags": [*B.CXXFLAGS, *defines], "files": result}
    text = json.dumps(record, indent=1, sort_keys=True)
    out.write_text(re.sub(r"\{[^{}]*\}", lambda m: re.sub(r"\s*\n\s*", " ", m.group(0)), text) + "\n")  # a kernel's numbers on one line
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
