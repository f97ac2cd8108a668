"""The 32-bit iteration sums on the host (tests/host_check/lk_fit_host.cpp, a g++ program with its own main):
(a) wave_sum2_fit_f32 and wave_sum2_f32 -- the text the CPU emulator runs -- equal (float)(int64 sum) bit for bit on the vectors of
    lk_fit_cases.h (random lanes; partial sums that wrap several times under totals inside +-(2^31 - 1); totals of exactly
    +-(2^31 - 1), 0, +-2^24 +- 1; one sum at the limit beside a small one), and equal wave_sum2_exact_f32 wherever its own
    precondition holds;
(b) lk_sums_fit is a proof: over random and adversarial 5 x 5, 13 x 13 and 21 x 21 templates (constant +-4080, a single spike, one
    magnitude with random signs, sums of squares placed within one f32 ulp of the threshold on both sides), wherever it says yes the
    exact integers 8160 * sum |Ixp| and 8160 * sum |Iyp| are below 2^31.  No case is skipped; at least a quarter of the templates
    lie on each side (the program's own assertion, repeated here on its numbers).
The second test is the same program under AddressSanitizer and UBSan -- a stand-alone child, nothing instrumented is loaded into
python: the wrapping adds are unsigned arithmetic, not signed overflow."""
import lk_fit


def _check(nums):
    n, n_wrap, n_templates, yes, no = nums
    print("lk_fit_host: %d vectors (%d with a wrapping partial sum); %d templates: %d fit, %d do not" % (n, n_wrap, n_templates, yes, no))
    assert n >= 1000 and n_wrap >= 400
    assert n_templates >= 15000 and yes + no == n_templates and 4 * yes >= n_templates and 4 * no >= n_templates


def test_fit_sums_and_predicate_on_the_host(tmp_path):
    _check(lk_fit.run(lk_fit.build_host(str(tmp_path)), str(tmp_path / "host.out")))


def test_fit_sums_and_predicate_under_sanitizers(tmp_path):
    _check(lk_fit.run(lk_fit.build_host(str(tmp_path), sanitize=True), str(tmp_path / "san.out")))
