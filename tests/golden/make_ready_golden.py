#!/usr/bin/env python3
"""Extract every Ready block the reference's interaction traces print into
tests/golden/ready_blocks.json.

    python tests/golden/make_ready_golden.py <path to the reference's raft/ directory>

Source: raft/testdata/*.txt (raft/interaction_test.go), read as text; nothing
of the reference is executed.  A Ready is printed by DescribeReady
(raft/util.go:89-120): "Ready MustSync=<bool>:", then, each only where
present, the SoftState line ("Lead:<id> State:<state>"), the HardState line
("HardState Term:<t> [Vote:<id> ]Commit:<c>", DescribeHardState: a Vote of 0
is not printed), "Entries:" and one "<term>/<index> Entry..." line per entry,
the "Snapshot Index:<i> Term:<t> ..." line, "CommittedEntries:" and its entry
lines, "Messages:" and the messages.  `stabilize` prints it indented below
"> <node> handling Ready", `process-ready <node>` unindented as the command's
output.

Output (data the reference printed, nothing else): per trace file a list of
blocks in file order, each
  line       1-based line of the "Ready MustSync" line in the file
  cmd_line   1-based line of the command whose output holds the block (the
             `line` of tests/golden/interaction_traces.json)
  node       the node that handled the Ready
  must_sync  bool
  soft       the SoftState line, or null
  hard       [term, vote, commit] (vote 0 = none), or null
  entries    [[term, index], ...] of "Entries:"
  committed  [[term, index], ...] of "CommittedEntries:"
  snapshot   the Snapshot's index, or null
TOTALS (asserted here and in tests/test_ready_model.py) are counted from the
testdata; the SoftState and HardState figures equal the number of "Lead:" and
"HardState " output lines in the ten files (31 and 66).
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TOTALS = {"blocks": 138, "must_sync": 58, "soft": 31, "hard": 66, "with_entries": 39,
          "entries": 75, "with_committed": 40, "committed": 74, "snapshot": 7}


def parse_file(lines):
    """The lines of one trace file -> its Ready blocks."""
    blocks, cur, section = [], None, None
    cmd_line, cmd_node, node = 0, None, None
    for no, raw in enumerate(lines, 1):
        line = raw.strip()
        if raw == "----":
            # the command is the non-comment block above
            j = no - 2
            while j >= 0 and lines[j] != "" and not lines[j].startswith("#"):
                j -= 1
            cmd_line = j + 2
            word = lines[j + 1].split()
            cmd_node = int(word[1]) if len(word) > 1 and word[1].isdigit() else None
            node, cur = cmd_node, None
            continue
        if line == "":
            cur = None
            continue
        h = re.match(r"^> (\d+) (receiving messages|handling Ready)$", line)
        if h:
            node, cur = int(h.group(1)), None
            continue
        m = re.match(r"^Ready MustSync=(true|false):$", line)
        if m:
            assert node is not None, f"line {no}: a Ready of no node"
            cur = {"line": no, "cmd_line": cmd_line, "node": node,
                   "must_sync": m.group(1) == "true", "soft": None, "hard": None,
                   "entries": [], "committed": [], "snapshot": None}
            blocks.append(cur)
            section = None
            continue
        if cur is None:
            continue
        if line.startswith("Lead:"):
            cur["soft"] = line
        elif line.startswith("HardState "):
            t = re.match(r"^HardState Term:(\d+)(?: Vote:(\d+))? Commit:(\d+)$", line)
            assert t, f"line {no}: {line}"
            cur["hard"] = [int(t.group(1)), int(t.group(2) or 0), int(t.group(3))]
        elif line == "Entries:":
            section = "entries"
        elif line == "CommittedEntries:":
            section = "committed"
        elif line.startswith("Snapshot Index:"):
            cur["snapshot"] = int(re.match(r"^Snapshot Index:(\d+) ", line).group(1))
            section = None
        elif line == "Messages:":
            section, cur = None, None
        elif re.match(r"^\d+/\d+ Entry\w+", line) and section:
            cur[section].append([int(x) for x in line.split()[0].split("/")])
    return blocks


def totals(files):
    b = [x for v in files.values() for x in v]
    return {"blocks": len(b), "must_sync": sum(x["must_sync"] for x in b),
            "soft": sum(x["soft"] is not None for x in b),
            "hard": sum(x["hard"] is not None for x in b),
            "with_entries": sum(bool(x["entries"]) for x in b),
            "entries": sum(len(x["entries"]) for x in b),
            "with_committed": sum(bool(x["committed"]) for x in b),
            "committed": sum(len(x["committed"]) for x in b),
            "snapshot": sum(x["snapshot"] is not None for x in b)}


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "testdata")):
        sys.exit(__doc__)
    data = os.path.join(sys.argv[1], "testdata")
    files = {}
    for name in sorted(os.listdir(data)):
        if name.endswith(".txt"):
            with open(os.path.join(data, name), encoding="utf-8") as f:
                files[name] = parse_file(f.read().split("\n"))
    got = totals(files)
    assert got == TOTALS, got
    with open(os.path.join(HERE, "ready_blocks.json"), "w", encoding="utf-8") as f:
        json.dump({"source": "raft/testdata/*.txt", "files": files}, f, indent=1)
    print("wrote", got)


if __name__ == "__main__":
    main()
