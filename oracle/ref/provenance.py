"""Writes oracle/_ref/provenance.json for the reference build (oracle/Makefile, target `ref`): the sha256
of every reference source file the harness units compiled (read from the compiler's dependency files),
the compiler's version line and the flags."""
from __future__ import annotations

import hashlib
import json
import subprocess
import sys
from pathlib import Path


def deps(dfile: Path) -> list[str]:
    text = dfile.read_text().replace("\\\n", " ")
    out = []
    for line in text.splitlines():
        if ":" in line:
            out += line.split(":", 1)[1].split()
    return out


def main() -> None:
    out, ref_src, cxx, flags, *dfiles = sys.argv[1:]
    root = Path(ref_src).resolve()
    files = set()
    for d in dfiles:
        for p in deps(Path(d)):
            rp = Path(p).resolve()
            if root in rp.parents:
                files.add(rp)
    sources = {str(p.relative_to(root)): hashlib.sha256(p.read_bytes()).hexdigest() for p in sorted(files)}
    version = subprocess.run([cxx, "--version"], capture_output=True, text=True, check=True).stdout.splitlines()[0]
    Path(out).write_text(json.dumps({"sources": sources, "compiler": version, "flags": flags.split()}, indent=1) + "\n")


if __name__ == "__main__":
    main()
