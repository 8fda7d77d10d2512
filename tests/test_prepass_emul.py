"""The pre-pass across its domain on the emulation build (tests/prepass_domain.py holds the builders, the model and the checks and
says why; tests/test_prepass_gpu.py runs a part of it on the HIP build): tgsf_align_windows as the pre-pass calls it against
edlib, the adapter identification, the quality encoding with the automatic -q and the automatic trims against the reference
binary.  Every case is first asserted, on a model here, to do what it is built for; the model is asserted against the reference's
own lines; then the emulated command line is compared with the reference.  The live cases need oracle/_ref/tgsfilter_ref and
skip without it; part 1 (then against the oracle's restatement of edlib) and the committed goldens do not."""
import os
import subprocess

import pytest

from tests import prepass_domain as pd

needs_ref = pytest.mark.skipif(not os.path.exists(pd.REF), reason="oracle/_ref/tgsfilter_ref not built (make -C oracle ref)")


@pytest.fixture(scope="module")
def emul():
    subprocess.run(["make", "-s", "-C", os.path.join(pd.ROOT, "tests", "emul")], check=True)
    return os.path.join(pd.ROOT, "tests", "emul", "libtgsf_emul.so")


@pytest.fixture(scope="module")
def cli():
    subprocess.run(["make", "-s", "-C", os.path.join(pd.ROOT, "tgsfilter_amd", "host"), "emul"], check=True)
    return pd.EMUL_CLI


# ---- 1: the library-shaped alignment call -------------------------------------------------------------------------------------
def test_k_is_the_c_expression_in_float32():
    assert pd.k_of(0.9) == [5, 5, 4, 4, 3, 3, 3, 3, 6, 6, 6, 6, 7, 7, 4, 4, 3, 3, 3, 3, 5, 5]
    assert [len(a) for a in pd.LIB] == [45, 45, 35, 35, 28, 28, 22, 22, 50, 50, 59, 59, 64, 64, 36, 36, 27, 27, 22, 22, 45, 45]
    assert all(pd.rev_comp(pd.LIB[a]) == pd.LIB[a ^ 1] for a in range(22))


def test_window_list_holds_what_it_is_there_for():
    pd.check_conditions()


@pytest.mark.parametrize("min_sim", pd.SIMS)
def test_emul_library_shaped_alignments(emul, min_sim):
    assert pd.check_windows(emul, min_sim) > 50000


def test_emul_one_call_of_the_products_size(emul):
    pd.check_product_sized_call(emul)


# ---- 2: the identification ----------------------------------------------------------------------------------------------------
def adapters_live(cli, case):
    pd.live(cli, case, pd.adapter_check(case))


@needs_ref
@pytest.mark.parametrize("copies", sorted(pd.CARRIERS))
@pytest.mark.parametrize("a", range(22))
def test_emul_entry_at_the_5p_end(cli, a, copies):
    adapters_live(cli, pd.five_case(a, copies))


@needs_ref
@pytest.mark.parametrize("a", range(22))
def test_emul_entry_at_the_3p_end_names_its_partner(cli, a):
    adapters_live(cli, pd.three_case(a))


@needs_ref
@pytest.mark.parametrize("a", range(22))
def test_emul_one_entry_at_each_end(cli, a):
    adapters_live(cli, pd.both_case(a))


@needs_ref
@pytest.mark.parametrize("a", sorted(pd.SIBLING_PINS))
def test_emul_siblings_as_the_reference_answers(cli, a):
    adapters_live(cli, pd.sibling_case(a))


@needs_ref
@pytest.mark.parametrize("below", (False, True), ids=("on", "below"))
@pytest.mark.parametrize("S", pd.DEPTH_SIMS)
@pytest.mark.parametrize("a", pd.DEPTH_ENTRIES)
def test_emul_depth_seam(cli, a, S, below):
    adapters_live(cli, pd.depth_case(a, S, below))


@needs_ref
@pytest.mark.parametrize("mirrored", (False, True))
@pytest.mark.parametrize("strong", (10, 11))
def test_emul_five_times_rule(cli, strong, mirrored):
    adapters_live(cli, pd.five_times_case(strong, mirrored))


@needs_ref
@pytest.mark.parametrize("name", pd.SAMPLING)
def test_emul_sampling(cli, name):
    adapters_live(cli, pd.sampling_case(name))


@needs_ref
@pytest.mark.parametrize("i,j", pd.CALL_SEAMS)
def test_emul_call_seam(cli, i, j):
    adapters_live(cli, pd.call_seam_case(i, j))


@needs_ref
@pytest.mark.parametrize("name", pd.BYTES)
def test_emul_bytes(cli, name):
    adapters_live(cli, pd.bytes_case(name))


@needs_ref
@pytest.mark.parametrize("fmt", pd.FORMATS)
def test_emul_input_formats(cli, fmt):
    adapters_live(cli, pd.format_case(fmt))


@needs_ref
@pytest.mark.parametrize("x", ("ont", "hifi", "clr"))
def test_emul_fallback_adapters_and_the_output(cli, x):
    def check(rc, err):
        pd.adapter_check(pd.fallback_case(x))(rc, err)
        assert len(pd.lines_with(err, "INFO: set NanoPore rapid adapter" if x == "ont" else "INFO: set PacBio blunt adapter")) == 1, err
    pd.live(cli, pd.fallback_case(x), check)


@pytest.mark.parametrize("name", sorted(pd.GOLDENS))
def test_emul_golden(cli, name):
    pd.check_golden(cli, name)


# ---- 3: the quality encoding and the automatic -q -----------------------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("lo", [l for l, _, _ in pd.ENCODING_LOW])
def test_emul_encoding_by_the_smallest_byte(cli, lo):
    case = pd.encoding_case(lo)
    pd.live(cli, case, pd.quality_check(case))


def test_encoding_cases_reach_all_three_branches():
    assert {b for _, _, b in pd.ENCODING_LOW} == {1, 2, 3}
    assert {(t, b) for _, t, b in pd.ENCODING_LOW} >= {(33, 3), (64, 3)}
    for lo, _, _ in pd.ENCODING_LOW:
        pd.encoding_case(lo)


def test_threshold_of_the_last_branch_is_never_met():
    """The last branch reads `min < 55`.  A smallest byte of 55 never gets there: the largest byte is then 55 .. 127 (qualities are
    compared as signed chars) and the first branch takes the pair.  So no input tells 55 from 56 in that branch, and none is here."""
    for lo in range(-128, 128):
        for hi in range(lo, 128):
            if pd.q_branch(lo, hi) == 3:
                assert lo != 55 and (lo < 55) == (lo < 56)
    assert pd.q_branch(255, 0) == 3 and pd.q_type(255, 0) == 64          # no read sampled: the scan's initial values


@needs_ref
@pytest.mark.parametrize("place", [p for p, _ in pd.ODD_PLACES])
def test_emul_encoding_looks_where_the_reference_looks(cli, place):
    case = pd.odd_byte_case(place)
    pd.live(cli, case, pd.quality_check(case))


@needs_ref
@pytest.mark.parametrize("x,maxq", [(x, m) for x, m, _ in pd.AUTO_Q])
def test_emul_automatic_q(cli, x, maxq):
    case = pd.auto_q_case(x, maxq)
    pd.live(cli, case, pd.quality_check(case))


@needs_ref
def test_emul_q_at_the_largest_quality_is_refused_by_both(cli):
    case = pd.fixed_q_case(30)
    pd.live(cli, case, pd.quality_check(case, refused=True), refused=True)
    case = pd.fixed_q_case(29)
    pd.live(cli, case, pd.quality_check(case))


@needs_ref
def test_emul_fasta_prints_no_encoding(cli):
    case = pd.format_case("fa")
    pd.live(cli, case, pd.quality_check(case, fasta=True))


# ---- 4: the automatic trims ---------------------------------------------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("kind", ("barcode", "same"))
@pytest.mark.parametrize("end", (5, 3))
@pytest.mark.parametrize("t", pd.PREFIX_T)
def test_emul_trim_of_a_fixed_prefix(cli, t, end, kind):
    case = pd.prefix_case(t, end, kind)
    pd.live(cli, case, pd.trim_check(case))


@needs_ref
@pytest.mark.parametrize("over", (0, 1))
@pytest.mark.parametrize("b,n", pd.BIAS_SEAMS)
def test_emul_trim_on_the_bias_seam(cli, b, n, over):
    case = pd.bias_case(b, n, over)
    pd.live(cli, case, pd.trim_check(case))


@needs_ref
@pytest.mark.parametrize("which,end", [(w, e) for w, e, _ in pd.CLAMPS if (w, e) != ("both", 5)])
def test_emul_clamp_of_the_5p_trim(cli, which, end):
    case = pd.clamp_case(which, end)
    pd.live(cli, case, pd.trim_check(case))


def test_emul_clamp_where_the_reference_races(cli):
    pd.check_clamp_where_the_reference_races(cli, pd.REF if os.path.exists(pd.REF) else None)
