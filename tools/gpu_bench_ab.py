"""Two checkouts of this repository (each built) alternating on one GPU: `bench.py --gpus 1 --steps K --warmup W` in A, then in B,
`--rounds` times, every run a fresh process with `other_configs` off; prints and writes every run's ms_per_step_median, both ranges
and whether every run of B lies below every run of A.
    python tools/gpu_bench_ab.py --a /path/to/parent --b . [--rounds 5] [--out profiles/rNN_ab_time.json] [-- extra bench.py arguments]"""
import argparse
import json
import os
import subprocess
import sys


def run(root, steps, warmup, extra, limit):
    env = dict(os.environ, EAVSR_BENCH_ALSO="")
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), *extra], cwd=root, env=env,
                       capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        raise SystemExit(f"bench.py in {root} ended with {r.returncode}:\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])["ms_per_step_median"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a", required=True)
    ap.add_argument("--b", required=True)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds one run may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("extra", nargs="*")
    args = ap.parse_args()
    runs = []
    for r in range(1, args.rounds + 1):
        a = run(args.a, args.steps, args.warmup, args.extra, args.limit)
        b = run(args.b, args.steps, args.warmup, args.extra, args.limit)
        runs.append({"round": r, "a_ms_per_step_median": round(a, 3), "b_ms_per_step_median": round(b, 3)})
        print(json.dumps(runs[-1]), flush=True)
    av, bv = [x["a_ms_per_step_median"] for x in runs], [x["b_ms_per_step_median"] for x in runs]
    out = {"command": f"bench.py --gpus 1 --steps {args.steps} --warmup {args.warmup} {' '.join(args.extra)}".strip(), "runs": runs,
           "a_range_ms": [min(av), max(av)], "b_range_ms": [min(bv), max(bv)], "a_spread_ms": round(max(av) - min(av), 3),
           "b_spread_ms": round(max(bv) - min(bv), 3), "separated": max(bv) < min(av),
           "difference_of_medians_ms": round(sorted(bv)[len(bv) // 2] - sorted(av)[len(av) // 2], 3)}
    print(json.dumps(out))
    if args.out:
        json.dump(out, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
