"""Basic blocks of one kernel instantiation, from the compiler's assembly listing: where the instructions of a stage are, how many
of them move values between the scalar file and spill lanes, and how often each block runs.

No GPU needed.  Compile the listing (the Makefile's flags, device side only; line tables add the source lines to the table and do
not change the code):

    hipcc $(make -s -C omg-planner_amd/csrc flags) --cuda-device-only -S -gline-tables-only \
          -Rpass-analysis=kernel-resource-usage omg-planner_amd/csrc/omg_kernels.hip -o omg_kernels.s 2> remarks.txt
    python tools/asm_blocks.py omg_kernels.s                       # k_goalset_queue<2,false,false,false,false,4>
    python tools/asm_blocks.py omg_kernels.s --path BB19_95,BB19_97x7 --json out.json

Per basic block (a label `.LBBn_m:` or a fall-through `; %bb.m:`): instructions, lane moves (v_readlane / v_writelane /
v_readfirstlane: SGPR spills live in the lanes of a VGPR, so a restore is a v_readlane and a store a v_writelane), which of the lane
moves address the spill registers (the VGPRs the listing declares as "SGPR spill to VGPR lane"), scalar loads, float64 VALU
instructions, LDS operations, the enclosing loop from the compiler's own loop comments, and the source lines of
omg_goalset_queue.h the block's instructions come from (with line tables).

Weights: blocks inside the main loop's tile / object loops are weighted with the per-workgroup counts of
profiles/r06f_block_counts.json (tiles visited, (tile, object) iterations) — found by the source line of the loop's header; every
other block has weight 1 per pass (how often a prologue block runs is read off the source: `--path` sums a hand-written path,
`LABELxN` = N passes).  The tool names ordinary instruction classes only.
"""
import argparse
import json
import re
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
DEFAULT_FN = "_Z15k_goalset_queueILi2ELb0ELb0ELb0ELb0ELi4EEv9ChunkArgs"
SRC = ROOT / "omg-planner_amd" / "csrc" / "omg_goalset_queue.h"
# loop headers of the main loop in the source -> the counter of profiles/*_block_counts.json that says how often their body runs
LOOP_MARKERS = [("for (int t = next_tile(); t >= 0; t = next_tile())", "tiles visited"),
                ("for (int o = h_ob; o < h_oe; ++o)", "(tile, object) iterations")]

LABEL = re.compile(r"^(\.LBB\d+_\d+):")
FALL = re.compile(r"^; %bb\.(\d+):")
LOOPC = re.compile(r"(?:Loop Header|in Loop): (?:Header=)?(BB\d+_\d+)?\s*Depth=(\d+)")
INSTR = re.compile(r"^\t([a-z][a-z0-9_]+)\b(.*)$")
LOC = re.compile(r"^\t\.loc\t(\d+) (\d+)")
FILE = re.compile(r'^\t\.file\t(\d+) "([^"]*)"(?: "([^"]*)")?')
SPILLREG = re.compile(r"implicit-def: \$vgpr(\d+) : SGPR spill to VGPR lane")


def function_text(text, fn):
    start = text.index(fn + ":")
    end = text.index(".Lfunc_end", start)
    return text[start:end].splitlines()


def parse(lines, file_ids):
    """-> (blocks, spill_vgprs).  A block: dict(name, loop, depth, n, lane_rd, lane_wr, spill_rd, spill_wr, rfl, sload, f64, lds, lines)."""
    spill = {f"v{m.group(1)}" for ln in lines for m in [SPILLREG.search(ln)] if m}
    blocks, cur, fn_no = [], None, None

    def new(name):
        b = dict(name=name, loop=None, depth=0, n=0, lane_rd=0, lane_wr=0, spill_rd=0, spill_wr=0, rfl=0, sload=0, f64=0, lds=0, salu=0, lines=set())
        blocks.append(b)
        return b

    cur_line = None
    for ln in lines:
        m = LABEL.match(ln)
        if m:
            cur = new(m.group(1)[2:])
            fn_no = cur["name"].split("_")[0]
        else:
            m = FALL.match(ln)
            if m:
                cur = new(f"{fn_no or 'BB?'}_{m.group(1)}" if fn_no else f"bb.{m.group(1)}")
        if cur is None:
            continue
        if (m or ln.lstrip().startswith(";")) and cur["n"] == 0:
            lc = LOOPC.search(ln)
            if lc and "Child Loop" not in ln and "Parent Loop" not in ln:
                cur["loop"], cur["depth"] = lc.group(1) or cur["name"], int(lc.group(2))
        lm = LOC.match(ln)
        if lm:
            cur_line = int(lm.group(2)) if int(lm.group(1)) in file_ids and int(lm.group(2)) > 0 else None
            continue
        im = INSTR.match(ln)
        if not im or im.group(1).startswith("s_nop") or im.group(1) == "s_waitcnt":
            continue
        op, rest = im.group(1), im.group(2)
        cur["n"] += 1
        if cur_line is not None:
            cur["lines"].add(cur_line)
        if op == "v_readlane_b32":
            cur["lane_rd"] += 1
            cur["spill_rd"] += any(r in spill for r in re.findall(r"\bv\d+\b", rest))
        elif op == "v_writelane_b32":
            cur["lane_wr"] += 1
            cur["spill_wr"] += rest.split(",")[0].strip() in spill
        elif op == "v_readfirstlane_b32":
            cur["rfl"] += 1
        elif op.startswith("s_load_") or op.startswith("s_buffer_load_"):
            cur["sload"] += 1
        elif op.startswith("ds_"):
            cur["lds"] += 1
        elif op.startswith("s_"):
            cur["salu"] += 1
        if op.startswith("v_") and re.search(r"_f64(_|$)", op):
            cur["f64"] += 1
    return blocks, spill


def loop_weights(blocks, counts, source=SRC):
    """weight per loop header label, from the source line its header block starts at"""
    if not counts:
        return {}
    src = Path(source).read_text().splitlines()
    out = {}
    for marker, key in LOOP_MARKERS:
        hits = [i + 1 for i, s in enumerate(src) if marker in s]
        if len(hits) != 1 or key not in counts:
            continue
        # the loop whose header block starts closest behind the `for` line (the header's own instructions belong to the body's first lines)
        heads = [(min(b["lines"]) - hits[0], b["name"]) for b in blocks if b["loop"] == b["name"] and b["lines"] and 0 <= min(b["lines"]) - hits[0] <= 25]
        if heads:
            out[min(heads)[1]] = counts[key] / counts.get("waves", 1.0)  # per wave of the workgroup
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("listing")
    ap.add_argument("--function", default=DEFAULT_FN, help="mangled name of the instantiation")
    ap.add_argument("--counts", default=str(ROOT / "profiles" / "r06f_block_counts.json"))
    ap.add_argument("--source", default=str(SRC), help="the omg_goalset_queue.h the listing was compiled from (line numbers of the loop headers)")
    ap.add_argument("--path", default="", help="comma-separated block names (LABEL or LABELxN) to sum, e.g. BB19_95,BB19_97x7")
    ap.add_argument("--lines", default="", help="only blocks with an instruction from these lines of omg_goalset_queue.h, e.g. 346-473")
    ap.add_argument("--json", default="", help="write the table here as well")
    a = ap.parse_args()
    text = Path(a.listing).read_text()
    file_ids = {int(m.group(1)) for ln in text.splitlines() if ln.startswith("\t.file") for m in [FILE.match(ln)]
                if m and "omg_goalset_queue.h" in (m.group(2) + "/" + (m.group(3) or ""))}
    blocks, spill = parse(function_text(text, a.function), file_ids)
    counts = {}
    if a.counts and Path(a.counts).exists():
        counts = json.loads(Path(a.counts).read_text()).get("per_goal_workgroup", {})
    lw = loop_weights(blocks, counts, a.source)
    # a block's weight: that of the innermost weighted loop around it (the compiler names the header of every enclosing loop only
    # for headers; for the others the innermost header is enough: inner loops of the main loop are listed behind their parent)
    parent = {}
    lines = function_text(text, a.function)
    for i, ln in enumerate(lines):
        m = LABEL.match(ln)
        if m and "Loop Header" in ln + (lines[i + 1] if i + 1 < len(lines) else ""):
            chain = [p for j in range(i, min(i + 6, len(lines))) for p in re.findall(r"Parent Loop (BB\d+_\d+)", lines[j])]
            parent[m.group(1)[2:]] = chain
    for b in blocks:
        w, lp = 1.0, b["loop"]
        if lp:
            for cand in [lp] + parent.get(lp, [])[::-1]:
                if cand in lw:
                    w = lw[cand]
                    break
        b["weight"] = w

    lo, hi = (int(x) for x in a.lines.split("-")) if a.lines else (0, 1 << 30)
    keys = ("n", "lane_rd", "lane_wr", "spill_rd", "spill_wr", "rfl", "sload", "salu", "f64", "lds")
    hdr = f"{'block':<12}{'loop':<12}{'d':>2}{'weight':>8}" + "".join(f"{k:>9}" for k in keys) + "  source lines"
    print(f"# {a.function}: {len(blocks)} blocks, spill registers {sorted(spill)}")
    print(hdr)
    tot = dict.fromkeys(keys, 0)
    rows = []
    for b in blocks:
        for k in keys:
            tot[k] += b[k]
        ls = sorted(b["lines"])
        if a.lines and not any(lo <= x <= hi for x in ls):
            continue
        span = f"{ls[0]}-{ls[-1]}" if ls else ""
        rows.append({**{k: b[k] for k in ("name", "loop", "depth", "weight") + keys}, "source": span})
        print(f"{b['name']:<12}{(b['loop'] or '-'):<12}{b['depth']:>2}{b['weight']:>8.2f}" + "".join(f"{b[k]:>9}" for k in keys) + f"  {span}")
    print(f"{'function':<34}" + "".join(f"{tot[k]:>9}" for k in keys))
    # the main loop per wave: every block with a weight from the counting build, times that weight
    loop = {k: sum(b[k] * b["weight"] for b in blocks if b["weight"] != 1.0) for k in keys}
    print(f"{'main loop x weight, per wave':<34}" + "".join(f"{loop[k]:>9.0f}" for k in keys))
    out = {"function": a.function, "spill_vgprs": sorted(spill), "totals": tot, "main_loop_weighted": loop, "blocks": rows}
    for key in ("; NumVgprs:", "; ScratchSize:", "; Occupancy:", "; TotalNumSgprs:"):
        i = text.index(key, text.index(a.function + ":"))
        out[key.strip("; :")] = int(re.match(r"\d+", text[i + len(key):].strip()).group(0))
    if a.path:
        byname = {b["name"]: b for b in blocks}
        psum = dict.fromkeys(keys, 0)
        for item in a.path.split(","):
            name, _, rep = item.strip().partition("x")
            for k in keys:
                psum[k] += byname[name][k] * (int(rep) if rep else 1)
        print(f"{'path':<34}" + "".join(f"{psum[k]:>9}" for k in keys))
        out["path"] = {"blocks": a.path, **psum}
    print({k: out[k] for k in ("NumVgprs", "TotalNumSgprs", "ScratchSize", "Occupancy")})
    if a.json:
        Path(a.json).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    sys.exit(main())
