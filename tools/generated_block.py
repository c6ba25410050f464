"""The plumbing the schedule generators (tools/gen_*_schedule.py) share: put a generated body between the
``// GENERATED-BEGIN`` / ``// GENERATED-END`` markers of a kernel source, or -- with ``--check`` -- verify that the committed
source already is what the tables generate (tests/test_abi_cpu.py runs every generator that way)."""
import re
import sys


def splice(src, body, tag=""):
    """`src` with the text between its GENERATED markers replaced by `body` (the marker lines stay).  A source with more than
    one generated block names the others: `tag` "-W4" means the markers ``// GENERATED-W4-BEGIN`` / ``// GENERATED-W4-END``."""
    new, n = re.subn(rf"(// GENERATED{tag}-BEGIN[^\n]*\n).*?([ \t]*// GENERATED{tag}-END)", lambda m: m.group(1) + body + "\n" + m.group(2), src, flags=re.S)
    assert n == 1, f"GENERATED{tag} markers not found"
    return new


def main(path, body, also_check=None, tagged=None):
    """Rewrite the block of `path`, or check it (--check; also_check(src) may return one more complaint).  `tagged`: {tag: body}
    of the source's further blocks (splice)."""
    src = open(path).read()
    new = splice(src, body)
    for tag, more in (tagged or {}).items():
        new = splice(new, more, tag)
    if "--check" in sys.argv:
        if new != src:
            raise SystemExit(f"{path}: the GENERATED block is out of date (run this script without --check)")
        complaint = also_check(src) if also_check else None
        if complaint:
            raise SystemExit(f"{path}: {complaint}")
        print("up to date", path)
        return
    open(path, "w").write(new)
    print("rewrote", path)
