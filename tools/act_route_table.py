"""The route table of the acting calls: which launches hl_forward, hl_forward_sequences and the four _dev acting calls make, per net,
SMARTIES_HIP_GENERIC, row or agent count and source -- status, error text, launches per timing label, training forwards and a SHA-256 of
the outputs (tests/act_routes.py: route_table, the function tests/test_hip_act_routes.py rebuilds the table with).  Recorded from the library
BEFORE a change of the host side that picks the routes, and held to entry by entry after it.

    python tools/act_route_table.py --out run_a.json              # one run on the GPU (--nets a,b: only those)
    python tools/act_route_table.py --out run_b.json              # ... and a second one, a process of its own
    python tools/act_route_table.py --merge run_a.json run_b.json # -> tests/act_routes_parent.json

--merge keeps the counters of every entry and drops the hash of an entry whose outputs differed between the two runs (it names them);
more than one entry in twenty without a hash is an error: the inputs are wrong then, not the cap."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import act_routes as acting  # noqa: E402


def dump(tables, path):
    """act_routes.route_pack's form, one line per group of entries: a change of one route is one line of a diff"""
    packed = acting.route_pack(tables)
    nets = ["  %s: [\n%s\n  ]" % (json.dumps(name), ",\n".join("    " + json.dumps(g, sort_keys=True, separators=(",", ":")) for g in groups))
            for name, groups in packed["nets"].items()]
    with open(path, "w") as f:
        hashes = ",\n".join(" " + ",".join(json.dumps(x) for x in packed["hashes"][i:i + 4]) for i in range(0, len(packed["hashes"]), 4))
        f.write('{\n"errors": %s,\n"hashes": [\n%s\n],\n"nets": {\n%s\n}\n}\n' % (json.dumps(packed["errors"], indent=1), hashes, ",\n".join(nets)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--nets", default="")
    ap.add_argument("--merge", nargs=2)
    a = ap.parse_args()
    if a.merge:
        A, B = [acting.route_unpack(json.load(open(p))) for p in a.merge]
        total = dropped = 0
        for name in A:
            assert sorted(A[name]) == sorted(B[name]), name
            for key, ea in A[name].items():
                eb = B[name][key]
                assert ea[:4] == eb[:4], ("status, error or counters differ between the runs", name, key, ea, eb)
                total += 1
                if ea[4] != eb[4]:
                    print("outputs differ between the two runs, hash dropped: %s %s" % (name, key))
                    ea[4] = None
                    dropped += 1
        print("%d entries, %d without a hash" % (total, dropped))
        assert 20 * dropped <= total, "more than one entry in twenty lost its hash"
        dump(A, a.out or acting.ROUTES_FILE)
        return
    from smarties_amd import load_hip
    api = load_hip()
    tables = {}
    for name in (a.nets.split(",") if a.nets else acting.ROUTE_NETS):
        tables[name] = acting.route_table(api, name)
        print("%s: %d entries" % (name, len(tables[name])), flush=True)
        dump(tables, a.out)


if __name__ == "__main__":
    main()
