"""The ``DDL_*`` surface: every name in the sources is in the ARCHITECTURE settings table, and the
table names nothing that is gone (no GPU, no library load)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOKEN = re.compile(r"DDL_[A-Z0-9_]+")
DIRS = ("csrc", "databricks_distributed_deep_learning_amd", "benchmarks", "scripts")
SOURCE_EXT = (".py", ".sh", ".hip", ".cpp", ".h", ".json")


def _tree_tokens():
    found = set()
    for d in DIRS:
        for base, dirs, files in os.walk(os.path.join(ROOT, d)):
            dirs[:] = [x for x in dirs if x not in ("__pycache__", "_native")]
            for f in files:
                if f.endswith(SOURCE_EXT):
                    with open(os.path.join(base, f), errors="replace") as fh:
                        found.update(TOKEN.findall(fh.read()))
    return found


def _table_tokens():
    with open(os.path.join(ROOT, "docs", "ARCHITECTURE.md")) as fh:
        text = fh.read()
    section = text.split("\n## Settings\n", 1)[1].split("\n## ", 1)[0]
    return {m.group(1) for m in re.finditer(r"^\| `(DDL_[A-Z0-9_]+)` \|", section, re.M)}


def test_settings_table_matches_the_tree():
    tree, table = _tree_tokens(), _table_tokens()
    assert table, "no settings table in docs/ARCHITECTURE.md"
    assert not tree - table, f"not in the settings table: {sorted(tree - table)}"
    assert not table - tree, f"in the settings table but nowhere in the tree: {sorted(table - tree)}"
