"""The launches of tests/test_gpu_ff_rows.py: (group, Case), every one at c = 320, run in both storage types and named
<group>.<form>.<dtype>.<case> (Case.form, Case.name).  Shared with tests/test_ff_ref_cpu.py, which checks on the CPU that the
restatement itself meets the criteria on every case and that each planted fault is rejected.

Inputs: oracle.weights.synth_input / synth_param with the scales of test_ff_geglu_fused (W1 and W2 x 2) and
b1 x ff_ref.B1_SCALE = 1: the b1-of-the-previous-chunk mutant is rejected on every case without scaling b1 up (narrowest: bf16
at hidden = 1280, 4.6 x the restatement's row measure against the margin of 2).

A chunk is 32 hidden units; the main loop of ff_geglu_kernel takes two per iteration and ends in an even or an odd tail; the W1
ring has 2 slots, the W2 + b1 ring 3.  A wave holds 32 rows, a block 128."""
from tests.ff_ref import LN_REGIMES, Case

CHUNK_COUNTS = (1, 2, 3, 4, 5, 6, 7, 8, 13, 40)
ROW_COUNTS = (1, 31, 32, 33, 96, 127, 128, 129, 257)
ROWS = 161                              # one full block, then a block of one full wave, one one-row wave and two empty waves


def build():
    cases = []
    # 1. chunk counts: every ring phase x tail form x "request chunk c + 2 or not" is reached by 1 .. 7; 8, 13 and 40 wrap more
    for k in CHUNK_COUNTS:
        cases.append(("chunks", Case(ROWS, 32 * k)))
    # 2. row edges at an odd (3 chunks) and an even (4 chunks) tail
    for hidden in (96, 128):
        for rows in ROW_COUNTS:
            cases.append(("rows", Case(rows, hidden)))
    # 3. forms at 5 chunks
    for residual in ("", "separate", "inplace"):
        for b2 in (True, False):
            cases.append(("forms", Case(ROWS, 160, residual=residual, b2=b2)))
    cases.append(("forms", Case(ROWS, 160, residual="x", ln="standard")))          # ldm/modules/attention.py: ff(norm3(x)) + x
    cases.append(("forms", Case(ROWS, 160, residual="", ln="standard")))
    # 4. LayerNorm regimes at 3 chunks, a separate residual of N(0, 1) (x as the residual would bury an offset row's
    #    feed-forward under 128)
    for regime in LN_REGIMES:
        cases.append(("ln", Case(ROWS, 96, ln=regime)))
    return cases


CASES = build()
# in place against out of place, bit for bit
INPLACE_PAIRS = [(Case(ROWS, 160, residual="inplace", b2=b2), Case(ROWS, 160, residual="separate", b2=b2)) for b2 in (True, False)]
# one-row launches of these rows of a 161-row launch carry the same bits: first / last lane of a wave, of a block, the one-row wave
SINGLE_ROWS = (0, 31, 32, 127, 128, 159, 160)
SINGLE_ROW_CASES = [Case(ROWS, 96), Case(ROWS, 128), Case(ROWS, 96, ln="mixed")]


def case_id(group, case, dtype_name):
    return f"{group}.{case.form}.{dtype_name}.{case.name}"
