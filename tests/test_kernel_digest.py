"""tools/kernel_resources.py's digest of a kernel's instruction text: what it ignores (comments, blank and alignment lines, the index of the function in
its file inside local labels) and what it does not (anything an instruction says).  Literal text, nothing compiled."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.kernel_resources import digest, kernel_bodies, normalise  # noqa: E402

A = """\
; %bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\tv_cmp_gt_i32_e32 vcc, 16, v0
\ts_and_saveexec_b64 s[2:3], vcc
\ts_cbranch_execz .LBB3_2
; %bb.1:                                ; %if.then
\tv_lshlrev_b32_e32 v1, 2, v0            ; comment a
\t.p2align\t6
.LBB3_2:                                ; %exit
\ts_endpgm
""".split("\n")

B = """\
; %bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\tv_cmp_gt_i32_e32 vcc, 16, v0

\ts_and_saveexec_b64 s[2:3], vcc
\ts_cbranch_execz .LBB17_2
; %bb.1:
\tv_lshlrev_b32_e32 v1, 2, v0            ; another comment
.LBB17_2:
\ts_endpgm
""".split("\n")


def test_function_index_and_comments_do_not_count():
    assert normalise(A) == normalise(B)
    assert digest(A) == digest(B)
    assert normalise(A)[3:6] == ["s_cbranch_execz .LBB_2", "v_lshlrev_b32_e32 v1, 2, v0", ".LBB_2:"]


def test_an_operand_counts():
    c = [ln.replace("v1, 2, v0", "v1, 3, v0") for ln in B]
    assert c != B and digest(c) != digest(B)
    d = [ln.replace(".LBB17_2", ".LBB17_3") for ln in B]          # the label's own number stays
    assert digest(d) != digest(B)


def test_a_kernel_runs_from_its_label_to_its_func_end():
    # (the kernel descriptor stands in front of .Lfunc_end and names the kernel: a renamed kernel with the same text compares equal)
    text = ("\t.globl\tk_a\nk_a:\n" + "\n".join(A) + "\n\t.amdhsa_kernel k_a\n\t.amdhsa_next_free_vgpr 2\n.Lfunc_end3:\n\t.size\tk_a, .Lfunc_end3-k_a\n\t.section\t.rodata\n"
            "k_b:\n" + "\n".join(B) + "\n\t.amdhsa_kernel k_b\n\t.amdhsa_next_free_vgpr 2\n.Lfunc_end17:\n")
    bodies = kernel_bodies(text)
    assert sorted(bodies) == ["k_a", "k_b"]
    assert normalise(bodies["k_a"])[:-2] == normalise(A) and normalise(bodies["k_a"])[-2:] == [".amdhsa_kernel <self>", ".amdhsa_next_free_vgpr 2"]
    assert digest(bodies["k_a"]) == digest(bodies["k_b"])
    assert digest(kernel_bodies(text.replace("free_vgpr 2\n.Lfunc_end17", "free_vgpr 3\n.Lfunc_end17"))["k_b"]) != digest(bodies["k_a"])
