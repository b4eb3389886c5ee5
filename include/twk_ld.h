// C++ API of the MI355X LD engine: the same class and settings struct a
// libtomahawk client uses (reference include/ld.h:40-69, include/core.h:909-924).
// A reference client switches by including this header (an `ld.h` shim that
// includes it is all a source tree needs) and linking
// libtomahawk_amd.so instead of libtomahawk.so.
#ifndef TWK_LD_H_
#define TWK_LD_H_

#include <cstdint>
#include <limits>
#include <string>
#include <vector>

namespace tomahawk {

// Process-global command line, defined by the executable (reference
// lib/main.cpp:4, include/tomahawk.h:34) and copied into the .two header
// (lib/ld/ld.cpp:610-612).  libtomahawk_amd only holds a weak reference to it: an
// executable that does not define it simply records an empty command line.
extern std::string LITERAL_COMMAND_LINE;

// Unpacking selector bits kept for source compatibility (core.h:84-88); the
// GPU engine always builds dense bit-planes in HBM.
#define TWK_LDD_NONE   0
#define TWK_LDD_VEC    1
#define TWK_LDD_LIST   2
#define TWK_LDD_BITMAP 4
#define TWK_LDD_ALL  ((TWK_LDD_VEC) | (TWK_LDD_LIST) | (TWK_LDD_BITMAP))

// Field-for-field twk_ld_settings (core.h:909-924; defaults core.cpp:297-306).
struct twk_ld_settings {
	twk_ld_settings();
	std::string GetString() const;

	bool square, window, low_memory, bitmaps, single;
	bool force_phased, forced_unphased, force_cross_intervals;
	int32_t c_level, bl_size, b_size, l_window;
	int32_t n_threads, cycle_threshold, ldd_load_type;
	int32_t l_surrounding;
	std::string in, out;
	double minP, minR2, maxR2, minDprime, maxDprime;
	int32_t n_chunks, c_chunk;
	std::vector<std::string> ival_strings;
	// Not in the reference: LD over a subset of the input's samples (`--keep FILE`, `--remove FILE`: one sample name per line, blank lines
	// and lines that start with '#' skipped; both: keep, then remove).  Every method that loads a .twk resolves the list against the
	// header before any device work (csrc/host/twk_sample_list.h: a name that is not in the header, a name twice in one file, an unreadable
	// file and an empty result are errors), loads the input as always and selects the samples on the GPU (twk_hip_select_samples); the
	// variants' Hardy-Weinberg P is recomputed over the kept samples, as a re-import of the subset would carry it.  The sample count and
	// the sample names of every output (.two header, PREFIX.samples.tsv, ##M_5_50) are then the kept samples', in header order.  Empty: all.
	std::string keep_file, remove_file;
	// Not in the reference: LD over a subset of the input's variants, PLINK's options in PLINK's order - samples first, then the
	// Hardy-Weinberg P over the kept samples, then the variants on those counts, then the compute.  `--extract FILE` / `--exclude FILE`: a
	// list of positions (csrc/host/twk_variant_list.h: CONTIG:POS or CONTIG<whitespace>POS per line, further columns ignored, positions
	// as the commands print them; every variant at a listed position matches; listed positions the input does not have are counted on
	// stderr; both: extract, then exclude).  `--maf` / `--max-maf` (minor allele frequency among the called alleles, bounds included),
	// `--mac` (minor allele count), `--geno` (the largest fraction of samples with a missing genotype), `--hwe` (the smallest
	// Hardy-Weinberg P): twk_hip_variant_filter's fields and rule.  The files are read before any device work; the variants are selected on
	// the GPU (twk_hip_select_variants), and the positions, per-variant side inputs (--assoc, --annot, the landscape) and the L / R split of
	// a -c / -C chunk follow the kept variants.  Refused where no one context holds the command's whole variant set (window mode over
	// several GPUs or processes) and in window mode under TWK_REF_COMPAT.  At their defaults: all variants.
	std::string extract_file, exclude_file;
	double min_maf = 0.0, max_maf = 0.5, max_missing = 1.0, min_hwe = 0.0;
	uint32_t min_mac = 0;
	bool selects_variants() const { return !extract_file.empty() || !exclude_file.empty() || min_maf != 0.0 || max_maf != 0.5 || min_mac != 0 || max_missing != 1.0 || min_hwe != 0.0; }
};

// What Score takes beyond twk_ld_settings.
struct twk_score_settings {
	std::string annot;          // the annotation file: with it the scores are partitioned, one column per category; empty: the plain score
	bool self = false;          // add the variant's own annotation to its partitioned scores (LDSC's convention, r2(v, v) = 1)
	int32_t top = 0;            // > 0: in place of the scores, every variant's `top` strongest partners (1 .. TWK_HIP_TOPK_MAX; not with annot)
	int32_t top_stat = -1;      // ... by the magnitude of this statistic (TWK_HIP_STAT_*; -1, not stated: r2)
};

// What Prune takes beyond twk_ld_settings.
struct twk_prune_settings {
	bool kept_only = false;     // write the kept variants' lines only (`prune --kept-only`): a list `--extract` reads back, PLINK's prune.in
};

// What Clump needs beyond twk_ld_settings.
struct twk_clump_settings {
	std::string assoc;          // the association file
	double p1 = 1e-4;           // index threshold: a variant with P <= p1 may start a clump
	double p2 = 1e-2;           // secondary threshold: a variant with P <= p2 may be claimed
};

// What Matrix needs beyond twk_ld_settings.
struct twk_matrix_settings {
	int stat = 0;               // TWK_HIP_STAT_R (signed r), _R2, _D or _DPRIME (include/twk_hip.h)
	float fill = 0.0f;          // the entry of a pair Compute would write no record for
	bool text = false;          // PREFIX.ld (space-separated text, as FINEMAP reads it) instead of PREFIX.npy
	bool band = false;          // band storage: per row only the columns inside the window (needs settings.window; no text form)
};

// What Decay needs beyond twk_ld_settings.
struct twk_decay_settings {
	int64_t range_bp = 10000000; // the distance the bins cover (the reference's default); the last bin also takes everything beyond it
	int32_t n_bins = 1000;       // the number of bins (the reference's default), at most 4096; range_bp / n_bins bases each
};

// What Aggregate prints per cell: the values of twk_aggregate_settings::reduce.
enum { TWK_AGGREGATE_MEAN = 0, TWK_AGGREGATE_COUNT = 1, TWK_AGGREGATE_MIN = 2, TWK_AGGREGATE_MAX = 3, TWK_AGGREGATE_SD = 4, TWK_AGGREGATE_TOTAL = 5 };

// What Aggregate needs beyond twk_ld_settings.
struct twk_aggregate_settings {
	int32_t x_bins = 1000, y_bins = 1000;  // bins per axis (the reference's defaults), 1 to 4096 each
	int32_t stat = 1;                      // TWK_HIP_STAT_R2; or _R (signed), _D, _DPRIME
	int32_t reduce = 0;                    // what is printed per cell: 0 mean, 1 count, 2 min, 3 max, 4 sd, 5 total
	int64_t min_count = 5;                 // a cell with fewer contributions prints 0 (the reference's -c)
};

// What Blocks takes beyond twk_ld_settings: the thresholds of Gabriel et al. (twk_hip_block_params, field for field) and the prefix of
// the files that keep the D' bounds (empty: not written).
struct twk_block_settings {
	uint32_t strong_lo = 70, strong_hi = 98, recomb_hi = 90, strong_lo_2 = 80, strong_lo_34 = 50, inform_permille = 950;
	uint32_t max_span_2 = 20000, max_span_3 = 30000;
	std::string ci_out;         // PREFIX of PREFIX.lo.npy, .hi.npy, .indptr.npy, .first.npy and .variants.tsv
};

// What Split takes beyond twk_ld_settings: the block sizes in variants, the largest number of blocks a contig is split into, and the
// number of blocks of the partition that is written out (0: none).
struct twk_split_settings {
	uint32_t min_size = 0, max_size = 0, max_blocks = 0;      // --min-size, --max-size, --max-blocks: all three required
	uint32_t blocks = 0;                                      // -B k: PREFIX.blocks.tsv holds every contig's k-block partition
};

// What Relationship needs beyond twk_ld_settings.
struct twk_relationship_settings {
	int32_t stat = 2;           // TWK_HIP_REL_KING; or _IBS (0), _IBS0 (1) (include/twk_hip.h)
	double fill = std::numeric_limits<double>::quiet_NaN();      // the entry of a sample pair whose denominator is 0
	bool text = false;          // with an output prefix: PREFIX.tsv (tab-separated text) instead of PREFIX.npy
};

class twk_ld {
public:
	twk_ld();
	~twk_ld();
	twk_ld(const twk_ld&) = delete;
	twk_ld& operator=(const twk_ld&) = delete;

	void operator=(const twk_ld_settings& s) { settings = s; }

	// ld.h:50-61.  Returns true on success; diagnostics go to std::cerr.
	bool Compute(const twk_ld_settings& settings);
	bool Compute();
	bool ComputeSingle(const twk_ld_settings& settings, bool verbose = false, bool progress = true);
	bool ComputeSingle(bool verbose = false, bool progress = true);
	// The reference's compile-time-gated micro-benchmark (ld.cpp:878-1057): not
	// available, returns false like a reference build without TWK_SLAVE_DEBUG_MODE.
	bool ComputePerformance();
	// Not in the reference: LD scores.  Loads the .twk exactly as Compute does (-I intervals, -w, -p / -u, -c / -C chunks as regions,
	// TWK_REF_COMPAT), and instead of records writes one text line per variant of the selection, in file order, to settings.out
	// ("-" or empty: stdout): contig, position (as `view` prints posA), the number of records Compute would write with the variant at
	// either end, and the sum of their R2 with 17 significant digits - reduced on one GPU (twk_hip_ld_score), no record is formed.
	// settings.minP must be 1 (the default).  `tomahawk ldscore` ends here.
	bool Score(const twk_ld_settings& settings);
	// ... and partitioned by the categories of score.annot, what stratified LD-score regression reads (LDSC's --l2 --annot): text, split on
	// tabs or spaces, `##` lines ignored; the first other line is the header, contig pos name1 .. nameC (a leading '#' is allowed; columns 3
	// and 4 named SNP and CM, as in LDSC's .annot, are skipped in every row), then one row per variant: contig name, position (1-based, as
	// Score prints it), C numbers, finite and at most 65536 in magnitude, 1 <= C <= 256.  Every variant of the selection at a (contig,
	// position) gets that row, variants the file does not name get zeros; the same key or name twice, a row of another length, a number that
	// is none or an unreadable file is an error, with file and line, before the input is opened or a device touched.  Per variant v and
	// category c the sum over v's partners w of a[w][c] * R2(v, w) is formed on one GPU (twk_hip_ld_score_annot: exact integer sums, the
	// same bits from run to run); score.self adds a[v][c] on the host.  Writes the `##` lines of Score, then ##annotations=C, ##M= and
	// ##M_5_50= (the categories' sums over the selection, and over its variants with a minor allele frequency above 0.05), ##self=1 with
	// score.self, and per variant contig, position, n_partners and the C scores with 17 significant digits.
	// With score.top = K > 0 (and no score.annot) the output is instead every variant's K strongest partners - proxy lookup - selected on one
	// GPU (twk_hip_ld_topk: |score.top_stat| descending as float32, ties to the partner earlier in the file): the `##` lines of Score, ##top=K,
	// ##stat=, with -c / -C a ##shard= line (the lists then hold the partners among that part's pairs only), and per variant and rank
	// contig, position, rank (from 1), the partner's contig and position, and the signed value with 9 significant digits.
	bool Score(const twk_ld_settings& settings, const twk_score_settings& score);
	// Not in the reference: greedy LD pruning in file order (PLINK's --indep-pairwise).  Loads the .twk exactly as Compute does (-I intervals,
	// -w, -p / -u, TWK_REF_COMPAT; the whole pair space: -c / -C are refused, the walk needs every pair) and writes one text line per
	// variant of the selection, in file order, to settings.out ("-" or empty: stdout): contig, position (as Score prints them) and keep,
	// 1 if no kept variant before it forms a record Compute would write with it, else 0 - decided and walked on one GPU
	// (twk_hip_ld_prune), no record is formed.  settings.minP must be 1 (the default).  `tomahawk prune` ends here.
	bool Prune(const twk_ld_settings& settings);
	// ... with prune.kept_only only the lines of the kept variants are written (the `##kept=` line stays): the file is a variant list that
	// `--extract` of any command reads back - PLINK's --indep-pairwise followed by --extract.
	bool Prune(const twk_ld_settings& settings, const twk_prune_settings& prune);
	// Not in the reference: LD clumping (PLINK's --clump).  Loads the .twk exactly as Prune does (-I intervals, -w, -p / -u, TWK_REF_COMPAT;
	// -c / -C are refused) and reads one association P value per variant from clump.assoc - text, split on tabs or spaces, lines that
	// start with '#' ignored: contig name, position (1-based, as Score and Prune print it), P (NA / nan: none), further columns ignored;
	// every variant of the selection at a (contig, position) gets that P, variants the file does not name get none; the same key twice,
	// a P outside [0, 1] or an unreadable file is an error before any device is touched.  The variants are visited in ascending P up to
	// clump.p1; one that belongs to no clump yet becomes an index variant and claims every free variant with P <= clump.p2 that forms a
	// record Compute would write with it - decided and walked on one GPU (twk_hip_ld_clump), no record is formed.  Writes one text line
	// per variant of the selection, in file order, to settings.out: contig, position, P, and contig and position of its index variant.
	// settings.minP must be 1 (the default).  `tomahawk clump` ends here.
	bool Clump(const twk_ld_settings& settings, const twk_clump_settings& clump);
	// Not in the reference: the dense LD matrix of the selection, the input of fine-mapping and of Bayesian polygenic scores.  Loads the
	// .twk exactly as Prune does (-I intervals, -w, -p / -u, TWK_REF_COMPAT; -c / -C are refused) and fills an n x n float32 matrix on one
	// GPU (twk_hip_ld_matrix): entry (u, v) is matrix.stat of the record Compute would write for the two variants - r carries D's sign -
	// and matrix.fill where it would write none; the diagonal is 1 (for D: the fill).  No record is formed.  settings.out is a PREFIX:
	// PREFIX.npy (NumPy format 1.0, '<f4', C order, shape (n, n)) or, with matrix.text, PREFIX.ld (one row per line, space-separated,
	// 9 significant digits), and always PREFIX.variants.tsv: one "contig <TAB> pos" line per row, as Score prints them.
	// settings.minP must be 1 (the default).  `tomahawk ldmatrix` ends here.
	// With matrix.band (settings.window must be set; matrix.text is refused) the same values leave in band storage
	// (twk_hip_ld_matrix_band): per row only the variants on its contig within settings.l_window bases, row_ptr[n] floats in place of
	// n * n - a chromosome-wide panel fits.  PREFIX.values.npy ('<f4', shape (nnz,)), PREFIX.indptr.npy ('<i8', shape (n + 1,)) and
	// PREFIX.first.npy ('<i4', shape (n,)): entry (u, v), first[u] <= v < first[u] + indptr[u + 1] - indptr[u], is
	// values[indptr[u] + v - first[u]]; both orientations are stored, so the three are a CSR matrix.  PREFIX.variants.tsv as above.
	bool Matrix(const twk_ld_settings& settings, const twk_matrix_settings& matrix);
	// LD decay: mean r2 by the distance between two variants (the reference's two_reader::Decay reads a .two file; here no record is
	// formed).  Loads the .twk exactly as Score does (-I intervals, -w, -p / -u, -c / -C chunks as regions, TWK_REF_COMPAT).  A pair counts
	// when Compute would write a record for it, both variants lie on one contig and their positions differ; its bin is
	// min(|posA - posB| / (decay.range_bp / decay.n_bins), decay.n_bins - 1).  Per bin the pairs are counted and their R2 summed on one GPU
	// (twk_hip_ld_decay: exact integer sums, the same bits from run to run).  Writes the `##` header lines and then the reference's
	// columns From, To, Mean, Frequency plus Sum (17 significant digits; Mean = Sum / Frequency, 0 for an empty bin), one line per bin,
	// to settings.out ("-" or empty: stdout).  settings.minP must be 1 (the default).  `tomahawk lddecay` ends here.
	bool Decay(const twk_ld_settings& settings, const twk_decay_settings& decay);
	// LD aggregate: the pairwise LD of the selection rasterised into x_bins * y_bins cells (the reference's two_reader::Aggregate reads a
	// .two file; here no record is formed).  Loads the .twk exactly as Score does (-I intervals, -w, -p / -u, -c / -C chunks as regions,
	// TWK_REF_COMPAT).  The landscape is the reference's rule applied to the loaded variants (csrc/host/twk_aggregate_landscape.h): one
	// contig - the data's range; several - every contig present at its header length; ceil((float)range / bins) bases a bin.  Every
	// record Compute would write adds its statistic to cell (x(A), y(B)) and to cell (x(B), y(A)) on one GPU (twk_hip_ld_aggregate: exact
	// integer sums, the same bits from run to run).  Writes `#` comment lines (x, y, bases per bin, range, every contig's offset) and
	// then x_bins rows of y_bins tab-separated values at 17 significant digits - the reduction of the cell, 0 below min_count - to
	// settings.out ("-" or empty: stdout).  settings.minP must be 1 (the default).  `tomahawk ldaggregate` ends here.
	bool Aggregate(const twk_ld_settings& settings, const twk_aggregate_settings& aggregate);
	// The sample relationship matrix: sample by sample over the variants of the selection (the reference's `relationship` walks the runs of a
	// .twk on the host; its numbers are not reproduced - include/twk_hip.h, twk_hip_relationship, says which of its quirks and why).  Loads the
	// .twk exactly as Prune does (-I intervals select whole blocks; no -c / -C) and fills an n x n float64 matrix over the header's samples on
	// one GPU: IBS (mean allele sharing), IBS0 or the KING-robust kinship, one IEEE division of exact integer counts per pair, rel.fill where
	// the denominator is 0.  settings.out empty or "-": the matrix as tab-separated text on stdout, one row per sample, 17 significant digits.
	// Else settings.out is a PREFIX: PREFIX.npy (NumPy format 1.0, '<f8', C order, shape (n, n)) or, with rel.text, PREFIX.tsv (the same text),
	// and always PREFIX.samples.tsv: one sample name per row, from the header.  `tomahawk relationship` ends here.
	bool Relationship(const twk_ld_settings& settings, const twk_relationship_settings& rel);
	// Not in the reference: haplotype blocks by the rule of Gabriel et al. (PLINK's --blocks, Haploview's default view).  Loads the .twk
	// exactly as Prune does (-I intervals, -p / -u, --keep, --extract ..; -c / -C are refused); the window is always on - settings.l_window
	// bases, 200,000 where settings.window is not set - and is also the longest block.  The D' confidence bounds of every pair Compute
	// would write a record for are formed and the blocks selected on one GPU (twk_hip_ld_blocks), no record is formed.  Writes the `##`
	// header lines and one line per block, in file order, to settings.out: contig, first position, last position, span in bases,
	// variants, strong pairs, recombinant pairs.  With blocks.ci_out the bounds are kept too (twk_hip_ld_dprime_ci_band, a second engine
	// call): PREFIX.lo.npy and PREFIX.hi.npy ('|u1', shape (nnz,); 255 where a pair has no record), PREFIX.indptr.npy, PREFIX.first.npy and
	// PREFIX.variants.tsv as Matrix writes them for a band.  Not PLINK's or Haploview's numbers: they add a LOD filter, their own MAF
	// rule and, unphased, a double-heterozygote term.  settings.minP must be 1 (the default).  `tomahawk blocks` ends here.
	bool Blocks(const twk_ld_settings& settings, const twk_block_settings& blocks);
	// Not in the reference: LD splitting (Prive 2021; bigsnpr's snp_ldsplit) - every contig of the selection cut into K near-independent
	// blocks of split.min_size .. split.max_size variants so that the r2 crossing a cut is smallest, for every K up to split.max_blocks.
	// Loads the .twk exactly as Prune does (-I, -p / -u, --keep, --extract ..; -c / -C are refused); the window (settings.l_window bases)
	// is required.  One engine call per contig (twk_hip_ld_split): the banded r2 matrix stays on the GPU and the dynamic programme runs
	// there.  settings.out is a PREFIX: PREFIX.costs.tsv holds per contig and feasible K the cost (the r2 outside the blocks, 17
	// digits), the cost as a fraction of the contig's total, and the sum of squared block sizes; with split.blocks = k,
	// PREFIX.blocks.tsv holds contig, block, first position, last position and variants of every contig's k-block partition - an error
	// if k is infeasible on some contig.  No max_r2 constraint, and not LDetect's rule.  settings.minP must be 1.  `tomahawk ldsplit`
	// ends here.
	bool Split(const twk_ld_settings& settings, const twk_split_settings& split);

	// Not in the reference: a switch of the GPU engine by name, applied to every engine context this object creates
	// (twk_hip_set_option, include/twk_hip.h - measurement and test switches; none changes a record), plus two of this
	// class's own: "force_device" (every context on GPU n: several contexts on one GPU), "progress_ms" (period of
	// the progress line) "map_output" (1: the .two is written through a shared mapping by the emitter's workers instead of a stream) and "emit_workers" (threads that
	// expand, compress and place the output blocks, per GPU; default min(-t, 32)) and "emit_backlog_mb" (expanded blocks that may wait in memory for those threads, per GPU;
	// default 0: six blocks per thread) and "emit_queue_pieces" (buffers of 2^20 survivors between the engine's thread and the emitter, per GPU; default 8, 0: none) and "record_codec" (1: output blocks compressed by the records' own zstd encoder instead of libzstd at level -k; default 0) and "direct_output" (1: block frames written with pwritev() and space reserved ahead instead of through the iostream; default 0).  `tomahawk calc --engine-option key=value` ends here.  Nothing is read from the environment
	// except TWK_HIP_DEVICE / TWK_HIP_GPUS / TWK_HIP_PART (placement), TWK_REF_COMPAT and TWK_HIP_NO_SCREEN.
	void SetEngineOption(const std::string& key, int64_t value);

	// Results of the last Compute(): pairs compared / records written (both copies).
	uint64_t n_pairs() const;
	uint64_t n_records() const;

private:
	class twk_ld_impl;
	twk_ld_settings settings;
	twk_ld_impl* mImpl;
};

}  // namespace tomahawk
#endif
