"""CPU only: tools/isa_diff.py, the proof that a header edit leaves the compiled-in kernels' machine code alone, must itself tell
"identical" from "changed".  The test commits a copy of the tool and of the kernel sources to a git repository of its own (the tree
under test need not be a checkout).  There `isa_diff.py HEAD 2 2 3` -- (2, 2, 3) is the cheapest unit with the full variant set --
finds no differing variant while the copy is unmodified, and finds some once ONE instruction of the single-chain ring block is changed."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_diff  # noqa: E402


@pytest.fixture(scope="module")
def checkout(tmp_path_factory):
    top = tmp_path_factory.mktemp("isa_diff_checkout")
    for rel in ["tools/isa_diff.py", "tinympc_amd/csrc/gen_units.py"] + ["tinympc_amd/csrc/" + name for name in isa_diff.SOURCES]:
        os.makedirs(top / os.path.dirname(rel), exist_ok=True)
        shutil.copy(os.path.join(ROOT, rel), top / rel)
    git = ["git", "-c", "user.name=test", "-c", "user.email=test@localhost", "-c", "commit.gpgsign=false"]
    for cmd in (["init", "-q"], ["add", "-A"], ["commit", "-q", "-m", "sources"]):
        subprocess.run(git + cmd, cwd=top, check=True, capture_output=True)
    return top


def _run(top):
    p = subprocess.run([sys.executable, str(top / "tools" / "isa_diff.py"), "HEAD", "2", "2", "3"], capture_output=True, text=True)
    m = re.search(r"^(\d+) of (\d+) variants of \(2, 2, 3\) differ from HEAD$", p.stdout, re.M)
    assert m, (p.stdout[-1000:], p.stderr[-2000:])
    return p.returncode, int(m.group(1)), int(m.group(2))


def test_unmodified_tree_is_identical_to_head(checkout):
    code, differing, total = _run(checkout)
    assert (code, differing) == (0, 0) and total > 0, (code, differing, total)


def test_one_changed_instruction_is_reported(checkout):
    header = checkout / "tinympc_amd" / "csrc" / "admm_kernel.hip.h"
    text = header.read_text()
    before = r'asm("s_nop 1\n\t" DPP_REP(K, RING1_COL)'
    assert text.count(before) == 1
    header.write_text(text.replace(before, before.replace("s_nop 1", "s_nop 2")))
    try:
        code, differing, total = _run(checkout)
    finally:
        header.write_text(text)
    assert code == 1 and 0 < differing <= total, (code, differing, total)


TILE_NAME = "tinympc_amd::admm_tile_kernel<2, 2, 4, 1, 1, 1, 0, 4, false, 0, false, 0>"


def test_names_mode_covers_a_runtime_instantiated_tile_form(checkout):
    """--names FILE: a cone form of the tile kernel, which no unit holds, compiled as an explicit instantiation -- identical while the
    copy is unmodified, reported once ONE instruction of the single-chain ring block its rows run is changed."""
    listing = checkout / "names.txt"
    listing.write_text("# one name per line\n%s\n" % TILE_NAME)

    def run():
        p = subprocess.run([sys.executable, str(checkout / "tools" / "isa_diff.py"), "HEAD", "--names", str(listing)], capture_output=True, text=True)
        m = re.search(r"^(\d+) of (\d+) variants of 1 names differ from HEAD$", p.stdout, re.M)
        assert m, (p.stdout[-1000:], p.stderr[-2000:])
        return p.returncode, int(m.group(1)), int(m.group(2))
    assert run() == (0, 0, 1)
    header = checkout / "tinympc_amd" / "csrc" / "admm_kernel.hip.h"          # (the tile kernel's rows run that header's ring blocks)
    text = header.read_text()
    before = r'asm("s_nop 1\n\t" DPP_REP(K, RING1_COL)'
    assert text.count(before) == 1
    header.write_text(text.replace(before, before.replace("s_nop 1", "s_nop 2")))
    try:
        assert run() == (1, 1, 1)
    finally:
        header.write_text(text)


def test_resource_directives_are_compared():
    unit = ("\t.globl\tk\nk:\n\ts_load_dword s0, s[4:5], 0x0 ; comment\n.LBB0_1:\n\ts_endpgm\n.Lfunc_end0:\n"
            "\t.amdhsa_kernel k\n\t\t.amdhsa_next_free_vgpr %d\n\t\t.amdhsa_private_segment_fixed_size 0\n\t.end_amdhsa_kernel\n")
    a, b = isa_diff.kernels(unit % 24), isa_diff.kernels(unit % 32)
    assert a["k"] == ["s_load_dword s0, s[4:5], 0x0", "s_endpgm", ".amdhsa_next_free_vgpr 24", ".amdhsa_private_segment_fixed_size 0"]
    assert [r[0] for r in isa_diff.compare(a, a)] == ["identical"] and [r[0] for r in isa_diff.compare(a, b)] == ["CHANGED"]
