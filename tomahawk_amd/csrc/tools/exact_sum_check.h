// The exact sums (csrc/hip/ld_exact_sum.h) played on the host, written once and run for both split widths in use (decay's 32, the
// aggregate's 20): decay_bin_check.cpp and aggregate_bin_check.cpp include this file inside their unnamed namespace, behind <cmath>,
// <cstdio>, <cstdint> and ld_exact_sum.h (through their kind's *_bin.h) at file scope, and call xs_check_all().  Every function goes against a naive restatement that shares no arithmetic with it:
//   the quantisation  by taking the double apart (frexp) and rounding its 53-bit integer mantissa, shifted, half to even, in integers;
//   the split         by a floor division and a non-negative remainder in 128-bit integers;
//   the conversion    by rounding the magnitude of the 128-bit integer to 53 bits, half to even, in integers, and scaling with ldexp.
// Covered: v = 0, +-1, one ulp beside +-1, the smallest doubles, ties at odd multiples of 2^-33 (neighbours, signs, what they round to),
// random sweeps; block sums of either sign through the split and back, alone and accumulated word by word; 128-bit sums on and beside a tie.
int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++failures <= 20) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rng() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

// value (an integer below 2^127) shifted right by k >= 0 bits, half to even
unsigned __int128 shift_right_half_even(unsigned __int128 v, int k) {
	if (k == 0) return v;
	if (k >= 127) return 0;
	const unsigned __int128 q = v >> k, rem = v - (q << k), half = (unsigned __int128)1 << (k - 1);
	if (rem > half || (rem == half && (q & 1))) return q + 1;
	return q;
}

// rint(|v| * 2^32), half to even, for 0 <= v
unsigned long long naive_quantise_magnitude(double v) {
	if (v == 0.0) return 0;
	int e = 0;
	const double m = frexp(v, &e);                                   // v = m * 2^e, 0.5 <= m < 1
	const unsigned long long mant = (unsigned long long)ldexp(m, 53);      // exact: 53 bits
	const int sh = e - 53 + 32;                                      // v * 2^32 = mant * 2^sh
	if (sh >= 0) return (unsigned long long)((unsigned __int128)mant << sh);
	return (unsigned long long)shift_right_half_even(mant, -sh);
}
// (half to even is symmetric: the magnitude is rounded, the sign put back)
long long naive_quantise(double v) { return v < 0 ? -(long long)naive_quantise_magnitude(-v) : (long long)naive_quantise_magnitude(v); }

double naive_to_double(__int128 q) {          // q / 2^32, rounded once
	if (q == 0) return 0.0;
	const bool neg = q < 0;
	unsigned __int128 v = neg ? (unsigned __int128)(-q) : (unsigned __int128)q;
	int bits = 0;
	for (unsigned __int128 x = v; x; x >>= 1) ++bits;
	int sh = bits > 53 ? bits - 53 : 0;
	unsigned __int128 top = shift_right_half_even(v, sh);
	if (top >> 53) { top >>= 1; ++sh; }                              // (the rounding carried into bit 53: a power of two)
	const double d = ldexp((double)(unsigned long long)top, sh - 32);
	return neg ? -d : d;
}

void check_value(double v) {
	const long long q = twk::xs_quantise(v), want = naive_quantise(v);
	CHECK(q == want, "quantise(%.17g) = %lld, want %lld", v, q, want);
	CHECK(fabs((double)q / twk::XS_SCALE - v) <= ldexp(1.0, -33), "quantise(%.17g) is more than 2^-33 away", v);
	const double sq = v * v;
	const unsigned long long q2 = twk::xs_quantise_sq(v), want2 = naive_quantise_magnitude(sq);
	CHECK(q2 == want2, "quantise_sq(%.17g) = %llu, want %llu", v, q2, want2);
	CHECK(twk::xs_quantise_sq(-v) == q2 && twk::xs_quantise(-v) == -q, "quantise(%.17g) is not symmetric", v);
	CHECK(twk::xs_value_to_double(q) == naive_to_double(q), "value_to_double(%lld)", q);
}

void check_quantise() {
	using namespace twk;
	const double ulp1 = ldexp(1.0, -52);
	for (double v : {0.0, 1.0, 1.0 - ulp1 / 2, 1.0 + ulp1, 1.0 + 4 * ulp1, 0.25, 0.5, 5e-324, 1e-300, 0.1, 0.2, 0.8, 1.0 / 3.0, ldexp(1.0, -32), ldexp(1.0, -33), ldexp(1.0, -34),
	                 ldexp(3.0, -34), nextafter(ldexp(1.0, -33), 0.0), nextafter(ldexp(1.0, -33), 1.0)})
		check_value(v);                                                // (check_value plays -v too)
	// ties: odd multiples of 2^-33 (exact doubles), what they round to, and both neighbours
	for (const uint64_t k : {0ull, 1ull, 2ull, 3ull, 4ull, 1000ull, 1001ull, 0x7FFFFFFFull, 0x80000000ull, 0xFFFFFFFEull, 0xFFFFFFFFull}) {
		const double tie = ldexp((double)(2 * k + 1), -33);
		check_value(tie); check_value(nextafter(tie, 0.0)); check_value(nextafter(tie, 2.0));
		CHECK((unsigned long long)xs_quantise(tie) == ((k & 1) ? k + 1 : k), "tie %llu -> %lld", (unsigned long long)k, xs_quantise(tie));
	}
	for (long long k = 1; k < 200; k += 2) {
		const double tie = ldexp((double)k, -33);
		check_value(tie); check_value(nextafter(tie, 0.0)); check_value(nextafter(tie, 2.0));
		const double big = ldexp((double)((1ll << 32) - k), -33);
		check_value(big); check_value(nextafter(big, 0.0)); check_value(nextafter(big, 2.0));
	}
	CHECK(xs_quantise(0.0) == 0 && xs_quantise(1.0) == (1ll << 32) && xs_quantise(-1.0) == -(1ll << 32) && xs_quantise(0.25) == (1ll << 30) && xs_quantise(-0.25) == -(1ll << 30), "the exact values");
	CHECK(xs_quantise(nextafter(1.0, 0.0)) == (1ll << 32) && xs_quantise(nextafter(1.0, 2.0)) == (1ll << 32), "one ulp beside 1");
	CHECK(xs_quantise(ldexp(1.0, -33)) == 0 && xs_quantise(ldexp(3.0, -33)) == 2 && xs_quantise(-ldexp(3.0, -33)) == -2 && xs_quantise(ldexp(5.0, -33)) == 2, "ties go to even");
	CHECK(xs_quantise_sq(0.5) == (1ull << 30) && xs_quantise_sq(-1.0) == (1ull << 32), "the exact squares");
	for (int k = 0; k < 200000; ++k) check_value((double)(rng() >> 11) * ldexp(1.0, -53) * (1.0 + ldexp(1.0, -40)));      // uniform in [0, 1 + a little)
	for (int k = 0; k < 2000; ++k) check_value(ldexp((double)(rng() >> 11), -53 - (int)(rng() % 40)));                   // small ones
	for (int k = 0; k < 2000; ++k) check_value(ldexp((double)(2 * (rng() >> 32) + 1), -33));                             // random ties
}

template <int K>
void check_split(long long s) {
	using namespace twk;
	const long long hi = xs_split_hi<K>(s);
	const unsigned long long lo = xs_split_lo<K>(s);
	// floor division and a non-negative remainder, in 128 bits
	const __int128 S = s, W = (__int128)1 << K;
	__int128 fq = S / W, fr = S % W;
	if (fr < 0) { fr += W; fq -= 1; }
	CHECK((__int128)hi == fq && (__int128)lo == fr, "split<%d>(%lld) = (%lld, %llu)", K, s, hi, lo);
	CHECK(lo < (1ull << K), "split<%d>(%lld): lo = %llu", K, s, lo);
	CHECK((__int128)hi * W + (__int128)lo == S && xs_join_signed<K>((unsigned long long)hi, lo) == S, "split<%d>(%lld) does not add up", K, s);
	CHECK(xs_sum_to_double_signed<K>((unsigned long long)hi, lo) == naive_to_double(S), "one block sum %lld through the split<%d> and back", s, K);
	if (s >= 0) {
		CHECK(xs_split_hi_u<K>((unsigned long long)s) == (unsigned long long)hi && xs_split_lo_u<K>((unsigned long long)s) == lo, "unsigned split<%d>(%lld)", K, s);
		CHECK(xs_sum_to_double_unsigned<K>((unsigned long long)hi, lo) == naive_to_double(S), "one unsigned block sum %lld through the split<%d> and back", s, K);
	}
}

// Many partial sums accumulated word by word, as the device's atomics do (wrapping 64-bit adds), against their sum in 128 bits: the
// split has no carry, so any way to cut a sum into blocks gives the same two-word total.
template <int K>
void check_accumulation(int count, long long magnitude, int sign_mode) {
	using namespace twk;
	unsigned long long acc_hi = 0, acc_lo = 0, uacc_hi = 0, uacc_lo = 0;
	__int128 total = 0;
	unsigned __int128 utotal = 0;
	for (int k = 0; k < count; ++k) {
		long long s = (long long)(rng() % (unsigned long long)magnitude);
		if (sign_mode == 1 || (sign_mode == 2 && (rng() & 1))) s = -s;
		acc_hi += (unsigned long long)xs_split_hi<K>(s); acc_lo += xs_split_lo<K>(s);
		total += s;
		const unsigned long long u = (unsigned long long)(s < 0 ? -s : s);
		uacc_hi += xs_split_hi_u<K>(u); uacc_lo += xs_split_lo_u<K>(u);
		utotal += u;
	}
	CHECK(xs_join_signed<K>(acc_hi, acc_lo) == total && xs_join_unsigned<K>(uacc_hi, uacc_lo) == utotal, "split<%d> sums of %d blocks below %lld (mode %d)", K, count, magnitude, sign_mode);
	CHECK(xs_sum_to_double_signed<K>(acc_hi, acc_lo) == naive_to_double(total), "%d signed sums below %lld (mode %d, split %d)", count, magnitude, sign_mode, K);
	CHECK(xs_sum_to_double_unsigned<K>(uacc_hi, uacc_lo) == naive_to_double((__int128)utotal), "%d unsigned sums below %lld (split %d)", count, magnitude, K);
}

template <int K>
void check_conversion() {
	using namespace twk;
	const __int128 W = (__int128)1 << K;
	// 128-bit sums against the hand-rounded conversion: beyond 2^64, exactly on and beside a rounding tie
	const unsigned long long his[] = {0ull, 1ull, (1ull << 20), (1ull << 21) - 1, (1ull << 21) + 1, (1ull << 33) + 1, 1ull << 40, (1ull << 43) + 1, (1ull << 57) - 1, 1ull << 56};
	const unsigned long long los[] = {0ull, 1ull, (1ull << 20) - 1, 1ull << 20, 0x80000000ull, 0xFFFFFFFFull, 1ull << 32, 0xFFFFFFFFFFull, (1ull << 63) - 1, (1ull << 63) + (1ull << 10),
	                                  (1ull << 63) + (1ull << 10) + 1, ~0ull};
	for (const unsigned long long hi : his) for (const unsigned long long lo : los) {
		const __int128 pos = (__int128)hi * W + (__int128)lo;
		CHECK(xs_sum_to_double_unsigned<K>(hi, lo) == naive_to_double(pos), "unsigned conversion<%d> of (%llu, %llu)", K, hi, lo);
		CHECK(xs_sum_to_double_signed<K>(hi, lo) == naive_to_double(pos), "signed conversion<%d> of (%llu, %llu)", K, hi, lo);
		const __int128 neg = -(__int128)hi * W + (__int128)lo;
		CHECK(xs_sum_to_double_signed<K>((unsigned long long)(-(long long)hi), lo) == naive_to_double(neg), "signed conversion<%d> of (-%llu, %llu)", K, hi, lo);
	}
	// the whole unsigned range of both words
	for (const unsigned long long hi : {~0ull >> 1, ~0ull}) {
		const __int128 v = (__int128)(((unsigned __int128)hi << K) + ~0ull);
		CHECK(xs_sum_to_double_unsigned<K>(hi, ~0ull) == naive_to_double(v), "unsigned conversion<%d> of (%llu, all ones)", K, hi);
	}
	for (int k = 0; k < 20000; ++k) {
		const unsigned long long hi = rng() >> (rng() % 64), lo = rng() >> (rng() % 64);
		const __int128 v = (__int128)(((unsigned __int128)hi << K) + lo);
		CHECK(xs_sum_to_double_unsigned<K>(hi, lo) == naive_to_double(v), "unsigned conversion<%d> of (%llu, %llu)", K, hi, lo);
	}
}

template <int K>
void check_width() {
	for (long long s : {0ll, 1ll, -1ll, (1ll << 20) - 1, 1ll << 20, -(1ll << 20), -(1ll << 20) - 1, -(1ll << 20) + 1, (1ll << K) - 1, 1ll << K, -(1ll << K), -(1ll << K) - 1, -(1ll << K) + 1,
	                    (1ll << 46), -(1ll << 46), -(1ll << 46) + 12345, (1ll << 39) - 1, -(1ll << 39) + 1, -(8192ll << 32), 8192ll << 32, 0x7FFFFFFFFFFFFFFFll, -0x7FFFFFFFFFFFFFFFll - 1})
		check_split<K>(s);
	for (int k = 0; k < 200000; ++k) { const long long s = (long long)(rng() >> (1 + rng() % 40)); check_split<K>(s); check_split<K>(-s); }
	// sums of block sums
	for (int mode = 0; mode < 3; ++mode) {
		check_accumulation<K>(1, 1ll << 46, mode);
		for (int k = 0; k < 200; ++k) check_accumulation<K>(50, 1ll << 46, mode);
		check_accumulation<K>(1000, 1ll << 46, mode);
		check_accumulation<K>(100000, 1ll << 46, mode);
		check_accumulation<K>(100000, 1ll << 39, mode);
		check_accumulation<K>(3000000, 1ll << 33, mode);
	}
	check_conversion<K>();
}

void xs_check_all() {
	check_quantise();
	check_width<20>();
	check_width<32>();
}
