"""How the inputs of an ill-conditioned shape of tests/blocks.py are chosen (CPU only): the fp32 and the fp64 build of the restatement
stepped side by side over a grid of (randSeed, synthetic replay seed) pairs; per pair the blocks over TOL32 / 3 and the margins on both
sides of that line -- the largest block below it, the smallest above.  A shape takes the pair with the widest margins whose blocks over
the line are bias blocks of W, few enough for the 1-in-20 cap of tests/test_blocks_cpu.py.

    python tools/block_seed_scan.py conv-atari-18opt-b8 [nRandSeeds nSynthSeeds]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import blocks  # noqa: E402


def scan(name, nRand, nSynth):
    base = blocks.SHAPES[name]
    line = blocks.TOL32 / 3
    print("%-6s %-6s %5s %5s  %-9s %-9s  blocks over TOL32 / 3" % ("rand", "synth", "over", "of", "max below", "min above"))
    for rs in range(1, nRand + 1):
        for ss in range(1, nSynth + 1):
            blocks.SHAPES["_scan"] = dict(kw=dict(base["kw"], randSeed=rs), sc=dict(base["sc"], seed=ss), n_eps=base["n_eps"])
            blocks.cpu_reference.cache_clear()
            ref = blocks.cpu_reference("_scan")
            worst = {}
            same = all(all((a["s32"][k] == a["s64"][k]).all() for k in blocks.INT_TAPS) for a in ref["steps"])
            for st in ref["steps"]:
                for q, devs in st["e_cpu"].items():
                    for b, v in devs.items():
                        if v != "zero":
                            worst[(q, b)] = max(worst.get((q, b), 0.0), v)
            over = {k: v for k, v in worst.items() if v > line}
            below = max(v for v in worst.values() if v <= line)
            print("%-6d %-6d %5d %5d  %.2e  %-9s  %s%s" % (rs, ss, len(over), len(worst), below, "%.2e" % min(over.values()) if over else "-",
                                                         " ".join("%s.%s" % k for k in sorted(over)), "" if same else "  (decisions differ)"), flush=True)
    del blocks.SHAPES["_scan"]


if __name__ == "__main__":
    scan(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 12, int(sys.argv[3]) if len(sys.argv) > 3 else 8)
