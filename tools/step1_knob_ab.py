"""A/B of (library, knobs) settings on Step 1, the way the Step-1 notes measure it: the settings alternate, one fresh process per setting and measurement, K alternations on
one box; stops at the first child that fails.  A setting is a name, a library path (empty: the in-tree library) and knobs for its processes (read behind
SHM_DEBUG_KNOBS=1, e.g. SHM_CONV_TIER_LOG, SHM_CONV_TIER_RING); the FIRST one is the baseline.  A measurement is `bench` (python bench.py, ms_per_step) or
file:hCoef:precision (Step 1 alone, shm_grid_run_conv, minimum of four: tools/ab.py's child).
    python tools/step1_knob_ab.py OUT ALTERNATIONS "bench,rocker.obj:4:64,..." "parent|lib/variants/parent/libshm_grid.so|" "G7r2||SHM_CONV_TIER_LOG=7;SHM_CONV_TIER_RING=2" ...
Every child's line goes to stdout and is appended to OUT as it comes; then a table: mean, min, max, spread (max - min) per setting and workload, the difference to the
baseline in ms, % and in units of the LARGER of the two spreads (nothing where a single alternation leaves no spread).  profiles/r09_*.txt were written by it."""
import json, os, re, subprocess, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
out_name, alts, kinds = sys.argv[1], int(sys.argv[2]), sys.argv[3].split(",")
settings = []
for a in sys.argv[4:]:
    name, lib, envs = a.split("|")
    settings.append((name, lib, dict(e.split("=", 1) for e in envs.split(";") if e)))
log = open(out_name, "a")


def say(s):
    print(s, flush=True)
    log.write(s + "\n")
    log.flush()


def run(cmd, lib, env):
    e = dict(os.environ, SHM_DEBUG_KNOBS="1", **env)
    e.pop("SHM_GRID_LIB", None)
    if lib:
        e["SHM_GRID_LIB"] = os.path.join(R, lib)
    p = subprocess.run(["timeout", "-k", "10", "150"] + cmd, env=e, capture_output=True, text=True, cwd=R)
    if p.returncode != 0:
        say("CHILD FAILED (%d): %s\n%s" % (p.returncode, " ".join(cmd), p.stderr[-800:]))
        sys.exit(1)
    return p.stdout


rows = {}
for k in range(alts):
    for name, lib, env in settings:
        for kind in kinds:
            if kind == "bench":
                o = run([sys.executable, "bench.py"], lib, env)
                res = json.loads([l for l in o.strip().split("\n") if l.startswith("{")][-1])
                st = res.get("step1", {})
                say("%-12s bench.py ms_per_step %.3f ms_conv %s pairs64 %s pairs32 %s redone %s" % (
                    name, res["ms_per_step"], res.get("phases_ms", {}).get("ms_conv"), st.get("pairs_fp64"), st.get("pairs_fp32"), st.get("pairs_redone")))
                rows.setdefault(("bench.py ms_per_step", name), []).append(float(res["ms_per_step"]))
                if k == 0 and name == settings[0][0]:
                    say("  keys: " + " ".join(sorted(res)) + " | step1: " + " ".join(sorted(st)) if isinstance(st, dict) else "")
            else:
                f, hc, prec = kind.split(":")
                line = run([sys.executable, "tools/ab.py", "--child", f, hc, prec, name], lib, env).strip()
                say(line)
                m = re.search(r"n=(\d+).* conv_alone ([\d.]+)", line)
                rows.setdefault(("Step 1 alone %s %s^3 fp%s" % (f, m.group(1), prec), name), []).append(float(m.group(2)))
base = settings[0][0]
say("\n%-44s %-12s %9s %8s %8s %8s  vs %s: ms, %%, gain in units of the larger spread" % ("workload", "setting", "mean ms", "min", "max", "spread", base))
for w in dict.fromkeys(k[0] for k in rows):
    b = rows[(w, base)]
    bm, bs = sum(b) / len(b), max(b) - min(b)
    for name, _, _ in settings:
        v = rows[(w, name)]
        vm = sum(v) / len(v)
        big = max(bs, max(v) - min(v))
        tail = "" if name == base else "   %+.3f  %+.2f %%" % (vm - bm, 100.0 * (vm - bm) / bm) + ("  %.1f x" % ((bm - vm) / big) if big > 0 else "")
        say("%-44s %-12s %9.3f %8.3f %8.3f %8.3f%s" % (w, name, vm, min(v), max(v), max(v) - min(v), tail))
