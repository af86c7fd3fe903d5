#!/usr/bin/env python3
"""Sweep of local_laplacian's frame-queue memory policy (MemPolicy, halide_amd/csrc/local_laplacian.hip above ld_frame4): which
flavour — plain, nt, sc1 — each access class of ll_down01e / ll_up0r / ll_down_strip2 should use on frame queues.

    python scripts/ll_mem_policy_sweep.py [--parent LIB] [--runs 3] [--out CALL.json] [name=]0xWORD ...
    python scripts/ll_mem_policy_sweep.py --report CALL1.json CALL2.json

A policy word has one hex digit per class (digit 0 = in_down ... digit 8 = l23_ld; 0 plain, 1 nt, 2 sc1).  Each word is a variant
library, halide_amd/lib/libhlmi_pol<hex>.so (make VARIANT=_pol<hex> EXTRA=-DHLMI_LL_POLICY=0x<hex>, at most 16 jobs), built here
when it is not there yet.  One invocation is one CALL: `--runs` rounds over the variants, and in a round every variant's run of
    bench.py --gpus 1 --steps 20 --warmup 3
follows a run of the parent's library (--parent; default: the product library, whose frame-queue policy is the committed default):
parent, variant 1, parent, variant 2, ...; a last parent run closes the call.  Every bench run is a process of its own under
`timeout -k 10`; a run that fails ends the sweep at once, nothing is repeated.

The rule a policy has to meet (--report over the files of two separate calls): in BOTH calls every run of the variant lies above
the parent's maximum of the same call.  The report prints per variant the runs, the median, the gain of the medians, the `paired`
gain (median over the variant's runs of run / mean of the parent runs before and after it: the box's clock state drifts within a
call, and the pair sees the same state), the parent's max - min of the same call and the verdict."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "halide_amd", "lib")
RUN_LIMIT_S = 240   # one bench.py run: set-up (8 synthetic 4K frames) + 23 steps of 128 frames, well under a minute


def variant_lib(word):
    return os.path.join(LIBDIR, f"libhlmi_pol{word:x}.so")


def build(word):
    lib = variant_lib(word)
    if not os.path.exists(lib):
        subprocess.run(["make", "-s", "-j16", "-C", os.path.join(ROOT, "halide_amd", "csrc"), f"VARIANT=_pol{word:x}",
                        f"EXTRA=-DHLMI_LL_POLICY=0x{word:x}"], check=True)
    return lib


def bench_once(lib):
    """`value` (Mpx/s on uniform noise) of one bench.py process with the library `lib`; exits the sweep if the run fails"""
    env = dict(os.environ, HLMI_LIB=lib)
    p = subprocess.run(["timeout", "-k", "10", str(RUN_LIMIT_S), sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                        "--steps", "20", "--warmup", "3"], env=env, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"bench.py with {lib} ended with status {p.returncode}: the sweep stops here")
    line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
    return json.loads(line)["value"]


def call(args):
    parent = os.path.abspath(args.parent)
    if not os.path.exists(parent):
        raise SystemExit(f"no parent library {parent}")
    policies = []
    for a in args.policies:
        name, _, w = a.rpartition("=")
        word = int(w, 16)
        policies.append((name or f"0x{word:09x}", word, build(word)))
    res = {"parent": parent, "parent_runs": [], "variants": {n: {"word": f"0x{w:09x}", "runs": []} for n, w, _ in policies}}

    def save():   # after every run: a call that is cut short keeps what it measured
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
    for r in range(args.runs):
        for n, w, lib in policies:
            res["parent_runs"].append(bench_once(parent))
            print(f"[round {r}] parent {res['parent_runs'][-1]:.1f}", flush=True)
            v = bench_once(lib)
            res["variants"][n]["runs"].append(v)
            res["variants"][n].setdefault("after_parent_run", []).append(len(res["parent_runs"]) - 1)
            print(f"[round {r}] {n} 0x{w:09x} {v:.1f}", flush=True)
            save()
    res["parent_runs"].append(bench_once(parent))
    print(f"[closing] parent {res['parent_runs'][-1]:.1f}", flush=True)
    save()
    report([res])


def report(calls):
    names = []
    for c in calls:
        names += [n for n in c["variants"] if n not in names]
    for i, c in enumerate(calls):
        pr = c["parent_runs"]
        runs = ' '.join(f'{v:.1f}' for v in pr) if len(pr) <= 8 else f"{len(pr)} (min {min(pr):.1f})"
        print(f"call {i + 1}: parent {os.path.basename(c['parent'])} runs {runs}  median {statistics.median(pr):.1f}  "
              f"max {max(pr):.1f}  max - min {max(pr) - min(pr):.1f}  (Mpx/s)")
    print(f"{'policy':22s} {'word':12s} {'runs per call':56s} {'median':>9s} {'vs parent':>10s} {'paired':>8s} {'parent max - min':>17s}  every run above the parent's max")
    for n in names:
        cells, verdicts, spreads, allruns, gains, paired = [], [], [], [], [], []
        word = ""
        for c in calls:
            v = c["variants"].get(n)
            if not v:
                cells.append("-")
                verdicts.append(None)
                continue
            word = v["word"]
            pr = c["parent_runs"]
            cells.append(" ".join(f"{x:.1f}" for x in v["runs"]))
            verdicts.append(min(v["runs"]) > max(pr))
            spreads.append(f"{max(pr) - min(pr):.1f}")
            allruns += v["runs"]
            gains.append(statistics.median(v["runs"]) / statistics.median(pr) - 1.0)
            paired += [x / ((pr[j] + pr[j + 1]) / 2) - 1.0 for x, j in zip(v["runs"], v.get("after_parent_run", []))]
        ran = [x for x in verdicts if x is not None]
        verdict = "not measured" if not ran else ("in " + " / ".join("-" if x is None else "yes" if x else "no" for x in verdicts))
        if len(calls) >= 2 and len(ran) == len(calls):
            verdict += "  -> PASSES" if all(ran) else "  -> fails"
        elif ran and not all(ran):
            verdict += "  -> fails"
        print(f"{n:22s} {word:12s} {' | '.join(cells):56s} {statistics.median(allruns):9.1f} {statistics.fmean(gains) * 100:+9.2f}% "
              f"{(f'{statistics.median(paired) * 100:+.2f}%' if paired else '-'):>8s} {' / '.join(spreads):>17s}  {verdict}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", default=os.path.join(LIBDIR, "libhlmi.so"), help="the library every variant is measured against")
    ap.add_argument("--runs", type=int, default=3, help="bench.py runs per library and call (at least 3)")
    ap.add_argument("--out", help="write this call's runs to a JSON file (for --report)")
    ap.add_argument("--report", nargs="+", metavar="CALL.json", help="print the table over the files of earlier calls and exit")
    ap.add_argument("policies", nargs="*", help="[name=]0xWORD")
    args = ap.parse_args()
    if args.report:
        return report([json.load(open(f)) for f in args.report])
    if args.runs < 3:
        ap.error("--runs must be at least 3")
    if not args.policies:
        ap.error("no policy words")
    call(args)


if __name__ == "__main__":
    main()
