"""The paged family's answers before a device is needed -- C entries and Python wrappers -- against the table recorded before their
argument rules were stated once (tests/paged_sweep.py says from which commit, and what a case is).  Host-only."""
import paged_sweep as ps

# The deliberate differences, by operation and case (never by asking the tree): what the recorded wrapper raised, what is required now.
# paged_decode had no rule for heads_kv = 0 and fell over its own `heads_q % heads_kv`; it now goes through the siblings' shape rules
# and raises their ValueError.  Nothing else may differ.
NOW = {
    ("py", "decode/heads_kv=0"): (["ZeroDivisionError", "integer division or modulo by zero"],
                                  ["ValueError", "heads_q (8) must be divisible by heads_kv (0)"]),
}


def test_paged_contract_matches_the_recorded_table():
    gold, got = ps.load_fixture(), ps.run()
    # the table is what the sweep defines, and it is not trivial
    assert list(gold["c"]) == sorted("%s/%d/%s" % c[:3] for c in ps.c_cases()) and len(gold["c"]) > 1000
    assert len(gold["py"]) > 190 and {k.split("/")[0] for k in gold["py"]} == {"decode", "query", "prefill", "cascade"}
    for kind, (_, size, entry) in ps.KINDS.items():
        base_rows = [gold["c"]["%s/%d/none" % (kind, b)] for b in ps.bases(kind)]
        assert len(base_rows) >= 2 and all(r[0] > 0 for r in base_rows if size), kind          # every valid base plans a workspace
        assert all(r[2] == [-1, "Library not initialized. Call aule_init() first."] for r in base_rows if entry), kind
        assert all(r[1][0] == 7 and r[1][1][2] >= 1 for r in base_rows if kind == "cascade")
    refusals = {r[2][1] for r in gold["c"].values() if r[2] and r[2][0] == -3}
    assert len(refusals) > 50 and sum(r[2] == [0, ""] for r in gold["c"].values() if r[2]) >= 40   # (the messages carry values)
    assert {v[0] for v in gold["py"].values()} == {"ValueError", "AuleError", "TypeError", "ZeroDivisionError"}
    want = {t: dict(gold[t]) for t in ("c", "py")}
    for (t, key), (was, now) in NOW.items():
        assert gold[t][key] == was, (t, key, gold[t][key])
        want[t][key] = now
    diff = ps.differences(want, got)
    for t, key, was, now in diff:
        print("%s %s\n  required %r\n  now      %r" % (t, key, was, now))
    assert not diff, "%d entries differ from the recorded table (printed above): %s" % (len(diff), [d[:2] for d in diff[:8]])
