"""Build an A/B variant of libmerging_hip.so from an edited temporary copy of csrc/ (the shipped
source has no compile-time knobs): each argument after the name is `old=>new`, a literal text
replacement that must match exactly once across merging_hip.hip and its parts (`old=>>new`: every
occurrence).

    python tools/ab_source.py ahead6 'kQGlobalAhead = 3;=>kQGlobalAhead = 6;'
    -> tools/variants/lib_ahead6.so (same flags as merging_gym/build.py)
"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "merging-gym_amd"))
from merging_gym import build  # noqa: E402


def edited_copy(src, edits, dst):
    """Copy the translation unit `src` and the parts it includes into the directory `dst`, apply
    `edits` -- (old, new, count) literal replacements, the matches counted across all the files;
    count None: every occurrence, at least one -- and return the copy's translation unit."""
    texts = {os.path.basename(p): open(p).read() for p in build.source_files(src)}
    for old, new, want in edits:
        n = sum(t.count(old) for t in texts.values())
        if n == 0 or (want is not None and n != want):
            raise SystemExit(f"'{old[:80]}' matches {n} times in {' '.join(texts)}")
        texts = {name: t.replace(old, new) for name, t in texts.items()}
    for name, t in texts.items():
        with open(os.path.join(dst, name), "w") as f:
            f.write(t)
    return os.path.join(dst, os.path.basename(src))


def compile_edited(src, edits, out):
    with tempfile.TemporaryDirectory() as td:
        tu = edited_copy(src, edits, td)
        subprocess.check_call([build.hipcc(), *build.HIPCC_FLAGS, "-I", build.INCLUDE, "-o", out, tu])
    print(out)


def patched_source(patch):
    """The single-file merging_hip.hip a tools/variants/*.patch records: the source at the commit its
    first line names (`# applies to <sha>`, the newest one it applies to) with the patch applied."""
    sha = open(patch).readline().split()[3]
    rel = "merging-gym_amd/csrc/merging_hip.hip"
    with tempfile.TemporaryDirectory() as td:
        os.makedirs(os.path.join(td, os.path.dirname(rel)))
        with open(os.path.join(td, rel), "w") as f:
            f.write(subprocess.run(["git", "-C", ROOT, "show", f"{sha}:{rel}"], capture_output=True, text=True,
                                   check=True).stdout)
        subprocess.run(["git", "apply", os.path.abspath(patch)], cwd=td, check=True)
        return open(os.path.join(td, rel)).read()


def compile_text(text, out, sha_tag):
    """One single-file source text -> out, with the product's flags (warnings off: a diagnostic build)."""
    with tempfile.TemporaryDirectory() as td:
        tu = os.path.join(td, "merging_hip.hip")
        with open(tu, "w") as f:
            f.write(text)
        subprocess.check_call([build.hipcc(), *build.HIPCC_FLAGS, "-w", f'-DMG_SRC_SHA="{sha_tag}"', "-I", build.INCLUDE,
                               "-o", out, tu])
    print(out)


def main(argv):
    name, edits = argv[0], []
    for e in argv[1:]:
        every = "=>>" in e  # `old=>>new`: replace every occurrence (at least one)
        old, new = e.split("=>>" if every else "=>", 1)
        edits.append((old, new, None if every else 1))
    os.makedirs(os.path.join(ROOT, "tools", "variants"), exist_ok=True)
    compile_edited(build.SRC, edits, os.path.join(ROOT, "tools", "variants", f"lib_{name}.so"))


if __name__ == "__main__":
    main(sys.argv[1:])
