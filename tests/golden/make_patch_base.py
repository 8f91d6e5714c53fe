"""Regenerates tests/golden/appcore_patch_base.json from an ipcr checkout.

For every file integration/go/appcore_core.patch changes, the fixture records the line count and SHA-256 of the
checkout's file, and, for every hunk, where it starts, how many original lines it covers and the SHA-256 of those
lines.  No source text of the checkout is stored: tests/test_go_shim_lint.py checks the patch's own pre-image of each
hunk against these hashes, so the patch is known to apply to that checkout without fuzz or offset.

    python tests/golden/make_patch_base.py /path/to/ipcr-checkout
"""
import hashlib
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PATCH = os.path.join(ROOT, "integration", "go", "appcore_core.patch")
OUT = os.path.join(HERE, "appcore_patch_base.json")


def lines_sha256(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def hunk_ranges(patch_text):
    """-> {path: [(old_start, old_len), ...]} from the patch's `--- a/<path>` and `@@ -s,l ...` headers"""
    out, cur = {}, None
    for ln in patch_text.splitlines():
        m = re.match(r"--- a/(\S+)", ln)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        m = re.match(r"@@ -(\d+)(?:,(\d+))? \+\d+(?:,\d+)? @@", ln)
        if m and cur is not None:
            out[cur].append((int(m.group(1)), int(m.group(2) or "1")))
    return out


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    checkout = sys.argv[1]
    files = {}
    for rel, hunks in hunk_ranges(open(PATCH).read()).items():
        lines = open(os.path.join(checkout, rel), encoding="utf-8").read().split("\n")
        if lines and lines[-1] == "":
            lines.pop()
        files[rel] = {"lines": len(lines), "sha256": lines_sha256(lines),
                      "hunks": [{"old_start": s, "old_len": n, "sha256": lines_sha256(lines[s - 1:s - 1 + n])}
                                for (s, n) in hunks]}
    with open(OUT, "w") as f:
        json.dump({"patch": "integration/go/appcore_core.patch", "files": files}, f, indent=1)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
