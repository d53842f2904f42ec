"""CPU lint: no reference source text in the tree.  oracle/_ref is built from the reference checkout by path; the
checkout itself is never copied.  Every tracked (or to-be-tracked) file under oracle/ and tests/ is compared line by
line with the reference's src/*.h and src/*.cpp: no non-trivial line (>= 40 characters after whitespace
normalisation) may equal one of theirs.  A lint, not a parity test: it skips only where the reference is absent."""
import os
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
REF_SRC = Path(os.environ.get("RLS_REF_SRC", "/root/reference")) / "src"    # as __graft_entry__.REF_SRC_DEFAULT
MIN_LEN = 40


def _norm(line: str) -> str:
    return " ".join(line.split())


def _tree_files():
    try:
        out = subprocess.run(["git", "-C", str(ROOT), "ls-files", "--cached", "--others", "--exclude-standard",
                              "oracle", "tests"], capture_output=True, text=True, check=True).stdout.split()
        return [ROOT / p for p in out]
    except (OSError, subprocess.CalledProcessError):        # a tree without git metadata: walk it
        return [p for d in ("oracle", "tests") for p in (ROOT / d).rglob("*")
                if p.is_file() and "_ref" not in p.parts and "build" not in p.parts and "__pycache__" not in p.parts]


def test_no_reference_line_in_tree():
    if not REF_SRC.is_dir():
        pytest.skip(f"reference checkout absent ({REF_SRC})")
    ref_lines = set()
    for p in list(REF_SRC.glob("*.h")) + list(REF_SRC.glob("*.cpp")):
        for line in p.read_text(errors="replace").splitlines():
            s = _norm(line)
            if len(s) >= MIN_LEN:
                ref_lines.add(s)
    assert ref_lines
    hits = []
    for p in _tree_files():
        if not p.is_file():
            continue
        try:
            text = p.read_text()
        except UnicodeDecodeError:
            continue
        for k, line in enumerate(text.splitlines(), 1):
            s = _norm(line)
            if len(s) >= MIN_LEN and s in ref_lines:
                hits.append(f"{p.relative_to(ROOT)}:{k}: {s}")
    assert not hits, "reference source lines in the tree:\n" + "\n".join(hits[:40])
