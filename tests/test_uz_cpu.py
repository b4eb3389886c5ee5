"""The (U, Z) form of the three-product contraction without a GPU: `make uz-check` - the conversion the screen kernel runs
(csrc/hip/ld_two_screen.h: uz_to_hh_s, uz_prefix_to_hh_s) against the products over every small genotype table, every prefix / suffix split and
zero-padded rows - and `make form-check` on LaunchForm::uz, both under AddressSanitizer and UBSan; the identities once more in NumPy; and the
new kernel's registers in the engine's gfx950 assembly."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _make(target):
    r = subprocess.run(["make", "-C", ROOT, target], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    return r.stdout


def test_uz_check_tables_splits_and_padded_rows():
    """Every 3 x 3 table of up to 7 samples (12,870 of them), every (prefix, suffix) pair of tables of up to 4 + 4 samples (495 x 495), rows of
    1, 31, 32, 33, 1000 and 4097 samples over every prefix of whole words: the shared conversion gives the products' HH and S, and
    screen3_keeps / screen3_prefix_keeps decide identically on both (a difference fails the tool)."""
    out = _make("uz-check")
    m = re.search(r"uz-check: (\d+) cases, (\d+) bad", out)
    assert m and int(m.group(2)) == 0, out[-2000:]
    assert int(m.group(1)) >= 12_870 + 495 * 495 + 8 * (1 + 1 + 1 + 32 + 32 + 160)
    for line in ("every 3 x 3 table of up to 7 samples", "every prefix and suffix table of up to 4 + 4 samples", "zero-padded rows of 1, 31, 32, 33, 1000 and 4097 samples"):
        assert line in out, out[-2000:]


def test_form_check_covers_the_uz_attribute():
    out = _make("form-check")
    m = re.search(r"form-check: (\d+) cases, (\d+) bad", out)
    assert m and int(m.group(2)) == 0, out[-2000:]
    assert "form-check: (U, Z) attribute: three-product launches through a matrix only, by option uz alone; the ladder does not know it" in out


@pytest.mark.parametrize("N", [1, 31, 32, 33, 1000, 4097])
def test_identities_on_bit_planes(N):
    """HH = hA + hB - popc(H_A | H_B) and S = qA + qB - popc((Q_A ^ Q_B) & ~(H_A | H_B)) on random and on correlated genotype rows, packed
    into 32-bit words with zero padding, over the whole rows and over every prefix of whole words."""
    rng = np.random.default_rng(N)
    W = -(-N // 32)
    for corr in (False, True):
        gA = rng.choice(3, size=N, p=[0.5, 0.3, 0.2])
        gB = np.where(rng.random(N) < 0.8, gA, rng.choice(3, size=N)) if corr else rng.choice(3, size=N, p=[0.2, 0.5, 0.3])

        def plane(mask):
            bits = np.zeros(W * 32, dtype=np.uint8)
            bits[:N] = mask
            return np.packbits(bits.reshape(W, 32), axis=1, bitorder="little").view("<u4").ravel()
        hA, qA, hB, qB = plane(gA == 1), plane(gA == 2), plane(gB == 1), plane(gB == 2)
        popc = lambda x: np.unpackbits(x.view(np.uint8)).reshape(len(x), 32).sum(axis=1).astype(np.int64)
        cum = lambda x: np.concatenate([[0], np.cumsum(popc(x))])
        u, z = cum(hA | hB), cum((qA ^ qB) & ~(hA | hB))
        hh, s = cum(hA & hB), cum(qA & (hB | qB)) + cum((hA | qA) & qB)
        assert np.array_equal(cum(hA) + cum(hB) - u, hh) and np.array_equal(cum(qA) + cum(qB) - z, s)
        assert hh[-1] == np.sum((gA == 1) & (gB == 1)) and s[-1] == np.sum((gA == 2) * (gB >= 1) * 1 + (gA >= 1) * (gB == 2) * 1)


def test_uz_kernels_fit_four_waves_a_simd():
    """k_count3_uz_list_t as `make hip` compiles it for gfx950, the launch's and its density sample's: no scratch, no spilled register, at most
    128 VGPRs - four waves a SIMD, as the three-product kernel beside it."""
    seen = {n: util.kernel_resources(b) for n, b in util.engine_kernels().items() if "k_count3_uz_list_t" in n}
    assert len(seen) == 2, sorted(util.engine_kernels())
    for name, (vgprs, scratch, spills) in seen.items():
        assert scratch == 0 and spills == 0 and vgprs <= 128, (name, vgprs, scratch, spills)
