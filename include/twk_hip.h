/*
 * twk_hip.h -- C ABI of the MI355X (gfx950) pairwise-LD engine.
 *
 * This is the drop-in boundary for the `tomahawk calc` hot path.  The
 * reference (mklarqvist/tomahawk) has no FFI of its own: its replacement point
 * is the per-thread block-pair loop `twk_ld_slave::Phased/Unphased`
 * (lib/ld/ld_engine.cpp:1898-2188) that calls one `twk_ld_engine` kernel per
 * variant pair (lib/ld/ld_engine.h:225, kernels ld_engine.cpp:185-1160) and
 * `PhasedMath`/`UnphasedMath` (ld_engine.cpp:1162-1740).  Each entry point
 * below names the reference interface it replaces.
 *
 * Conventions: plain C types only; every function returns 0 (TWK_HIP_OK) or a
 * negative TWK_HIP_E_* code and never throws; the caller owns every host
 * buffer; the library owns all device memory inside the ctx; one ctx per
 * device, used from one host thread at a time.  There is NO CPU fallback: if
 * no HIP device is usable the calls fail with TWK_HIP_E_DEVICE.
 */
#ifndef TWK_HIP_H_
#define TWK_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: twk_hip_timing grew (fused / carrier-list counters); new entry points twk_hip_set_device_sink,
 *    twk_hip_device_records, twk_hip_fisher_exact.  A caller built against another version must not pass
 *    its structs in: compare twk_hip_abi_version() with the header it was compiled with. */
/* 3: twk_hip_set_option / twk_hip_get_option; the library no longer reads environment variables. */
/* 4: twk_hip_timing grew (three-product launches); option "three". */
/* 5: twk_hip_generate_synthetic_planted / twk_synth_planted_bitvector / twk_synth_plant_source (synthetic input with planted LD pairs);
 *    twk_hip_option_describe; twk_hip_timing grew (finish_ms); twk_hip_gather_records / twk_hip_gather_backend /
 *    twk_hip_drain_device_sink (the RCCL gather of a one-process multi-GPU run). */
/*    (still 5: twk_hip_ld_score - LD scores - is an entry point more; no struct and no existing entry point changed) */
/*    (still 5: twk_hip_ld_prune / twk_hip_prune_last - LD pruning - are two entry points more; no struct and no existing entry point changed) */
/*    (still 5: twk_hip_ld_clump / twk_hip_clump_last - LD clumping - are two entry points more; no struct and no existing entry point changed) */
/*    (still 5: twk_hip_ld_matrix / twk_hip_matrix_last - the dense LD matrix - are two entry points more; no struct and no existing entry point changed) */
/*    (still 5: twk_hip_ld_decay - LD decay - is an entry point more; no struct and no existing entry point changed) */
/*    (still 5: twk_hip_ld_aggregate - the LD aggregate - is an entry point more; no struct and no existing entry point changed) */
/*    (still 5: twk_hip_relationship / twk_hip_relationship_last - the sample relationship matrix - are two entry points more; no struct and no existing entry point changed) */
/*    (still 5: twk_hip_ld_score_annot - partitioned LD scores - is an entry point more; no struct and no existing entry point changed) */
/*    (still 5: twk_hip_bandmat_layout / twk_hip_ld_matrix_band / twk_hip_bandmat_last - the banded LD matrix - are three entry points more; no struct and no existing entry point changed) */
/*    (still 5: twk_hip_ld_dprime_ci_band / twk_hip_ld_blocks / twk_hip_blocks_last / twk_hip_blocks_stages - haplotype blocks - are four entry points and one struct more; nothing existing changed) */
/*    (still 5: twk_hip_ld_split / twk_hip_split_last - LD splitting - are two entry points more; no struct and no existing entry point changed) */
/*    (still 5: twk_hip_ld_topk / twk_hip_topk_last - top-k LD partners - are two entry points more; no struct and no existing entry point changed) */
/*    (still 5: twk_hip_select_samples / twk_hip_selection / twk_hip_get_meta / twk_hip_set_hwe / twk_hip_select_last - sample subsets - are five entry points more; no struct and no existing entry point changed) */
/*    (still 5: twk_hip_select_variants / twk_hip_variant_selection / twk_hip_variant_map / twk_hip_select_variants_last - variant subsets - are four entry points more; no existing struct and no existing entry point changed) */
#define TWK_HIP_ABI_VERSION 5

enum {
	TWK_HIP_OK         =  0,
	TWK_HIP_E_INVALID  = -1, /* bad argument */
	TWK_HIP_E_NOMEM    = -2, /* host or device allocation failed */
	TWK_HIP_E_DEVICE   = -3, /* HIP runtime error / no device */
	TWK_HIP_E_OVERFLOW = -4, /* record buffer too small; *n_out holds the required count */
	TWK_HIP_E_STATE    = -5  /* call sequence error (e.g. compute before upload) */
};

/* Pair math selection; mirrors twk_ld_settings.force_phased / forced_unphased
 * (include/core.h:916) and the default per-pair rule of
 * twk_ld_slave::Calculate (ld_engine.cpp:2775,2803). */
enum {
	TWK_HIP_MODE_PHASED   = 1, /* calc -p : PhasedListVector/PhasedVectorized + PhasedMath   */
	TWK_HIP_MODE_UNPHASED = 2, /* calc -u : UnphasedVectorized(NoMissing) + UnphasedMath      */
	TWK_HIP_MODE_AUTO     = 3  /* calc    : unphased iff either variant has missing alleles   */
};

typedef struct twk_hip_ctx twk_hip_ctx;

/* Per-variant metadata: the fields of twk1_t (include/core.h:291-295) that the
 * pair loop and the math read (ac, an, pos, rid, hwe, gt_missing). */
typedef struct {
	uint32_t ac;      /* ALT allele count                       */
	uint32_t an;      /* number of MISSING alleles (sic)        */
	uint32_t pos;     /* 0-based position                       */
	uint32_t rid;     /* contig id                              */
	uint32_t missing; /* twk1_t.gt_missing (variant has a mask) */
	uint32_t _pad;
	double   hwe;     /* Hardy-Weinberg P                       */
} twk_hip_variant_meta;

/* Output filters: twk_ld_settings.minR2/maxR2/minDprime/maxDprime/minP
 * (include/core.h:921; defaults lib/core.cpp:304). */
typedef struct {
	double minR2, maxR2, minDprime, maxDprime, minP;
} twk_hip_filters;

/* A rectangular slice of the variant-pair space, in variant indices as
 * uploaded.  Replaces one ticket of twk_ld_dynamic_balancer::GetBlockPair
 * (lib/ld/ld_balancing.h:214-233): rows [rowA0,rowA0+nA) x cols [rowB0,rowB0+nB).
 * When diag != 0 (requires rowA0 == rowB0, nB >= nA) only pairs with col > row
 * are evaluated (ticket type 1, ld_engine.cpp:1913-1933); the columns beyond nA
 * form the rectangle to the right of the diagonal square. */
typedef struct {
	uint32_t rowA0, nA, rowB0, nB;
	int32_t  diag;
	int32_t  window;   /* option bits, see TWK_HIP_OPT_*                                */
	uint32_t l_window; /* base pairs (twk_ld_settings.l_window)                         */
	uint32_t one;      /* set by the planner only, read by the region walk that owns the plan only (0 from every caller): a launch
	                      in front of its rows' one_end, which may contract one product a pair                    */
} twk_hip_tile_desc;

/* Option bits for twk_hip_tile_desc.window and the `window` argument of ld_all / ld_region. */
enum {
	TWK_HIP_OPT_WINDOW      = 1, /* keep only same-contig pairs with |posA-posB| <= l_window (calc -w) */
	TWK_HIP_OPT_KEEP_LOW_AC = 2  /* do not skip pairs with ac_A + ac_B <= 2: the single-site loop has the
	                                skip commented out (ld_engine.cpp:2267-2269, 2293-2295)            */,
	TWK_HIP_OPT_REF_COMPAT  = 4  /* reproduce what the reference's PhasedVectorized really returns for pairs with
	                                missing genotypes when 2N is not a multiple of 128: its scalar tail adds the
	                                (A ref, B alt) count to REFREF and swaps the two off-diagonal cells, and REFREF is
	                                reduced by half the padding (ld_engine.cpp:596-609).  Off by
	                                default: the engine returns the correct table. */,
	TWK_HIP_OPT_R2_SCREEN   = 8  /* whole-triangle runs with filters.minR2 >= 0.001: decide from the two allele counts alone
	                                which pairs can reach the r2 cut-off at all (|D| <= a(1-b) for minor allele frequencies
	                                a <= b, so r2 <= a(1-b)/((1-a)b)), walk the variants in order of minor allele count and
	                                never contract the tiles outside that band.  Same records as without it (pairs in the
	                                band still go through the reference's formula); on cohort data, where most variants
	                                are rare, most pairs fall outside the band.  This is the engine's answer to the
	                                reference's O(carriers) list kernels for rare variants (twk_igt_list,
	                                include/core.h:517-672, PhasedListVector ld_engine.cpp:185-267): not a faster way to
	                                count a rare pair, a proof that it need not be counted.  Off by default at the ABI
	                                (bench.py measures the full contraction); `tomahawk calc` switches it on. */
};

/* One surviving pair, device-compacted.  Field-for-field the payload of
 * twk1_two_t (include/core.h:826-833) with variant indices instead of
 * rid/pos (the host expands them and writes the forward + reverse copies,
 * ld_engine.cpp:1290-1298). */
typedef struct {
	uint32_t idxA, idxB; /* variant indices as uploaded           */
	uint32_t flags;      /* twk1_two_t.controller                 */
	uint32_t _pad;
	double   cnt[4];     /* REFREF, ALTREF-slot, REFALT-slot, ALTALT (core.h:833) */
	double   D, Dprime, R, R2, P, ChiSqFisher, ChiSqModel;
} twk_hip_record;

/* ---- device / context ------------------------------------------------- */
int twk_hip_abi_version(void);
int twk_hip_device_count(void);
const char* twk_hip_strerror(int code);
/* Last HIP runtime error text recorded on this ctx ("" if none). */
const char* twk_hip_last_error(const twk_hip_ctx* ctx);
int twk_hip_ctx_create(int device, twk_hip_ctx** out);
int twk_hip_ctx_destroy(twk_hip_ctx* ctx);

/* Page-locked host memory for upload staging (hipHostMalloc / hipHostFree): uploads from it run at
 * full PCIe rate and without a bounce copy.  No reference counterpart (the reference never leaves
 * host memory). */
int twk_hip_host_alloc(size_t bytes, void** out);
int twk_hip_host_free(void* p);

/* ---- input ------------------------------------------------------------ */
/* Declare the problem: n_samples diploid samples, n_variants variants.
 * Replaces twk_ld_engine::SetSamples (ld_engine.cpp:55-71) + the ldd block
 * arrays (ld.cpp:390-391). Frees any previous data. */
int twk_hip_set_problem(twk_hip_ctx* ctx, uint32_t n_samples, uint32_t n_variants);

/* Upload variants [first, first+count) as reference-layout bitvectors
 * (twk_igt_vec, include/core.h:724-753 built by core.cpp:349-438): for sample
 * s bit 2s = first allele is ALT, bit 2s+1 = second allele is ALT, little-
 * endian uint64 words, stride64 words per variant (>= ceil(2N/64)).  `mask`
 * may be NULL (no variant has missing data); otherwise same layout with both
 * bits of a sample set when either allele is missing (core.cpp:379-380).
 * Replaces twk1_ldd_blk::Inflate (ld_structs.cpp:125-203). */
int twk_hip_upload_bitvectors(twk_hip_ctx* ctx, uint32_t first, uint32_t count,
                              const uint64_t* data, const uint64_t* mask, size_t stride64,
                              const twk_hip_variant_meta* meta);

/* The same upload with the expansion done on the device: `bytes` holds the run-length genotype words of
 * `count` variants exactly as they are stored in a .twk block (twk1_t::gt, include/core.h:195-205:
 * 1, 2 or 4 bytes per run, little endian, run = length << (2+2m) | A << (1+m) | B with m = 1 and two bits
 * per allele when the variant has missing genotypes), desc[i] says where variant first+i's runs start.
 * A HIP kernel does what twk_igt_vec::Build does on the reference's unpack threads
 * (lib/core.cpp:349-391, lib/ld/ld_unpacker.h:44-123): bitvector + mask, padding bits zero - so the
 * PCIe link carries the compressed genotypes, not N/4 bytes per variant.  `bytes` may be pageable or
 * pinned host memory and is free for reuse when the call returns.  Runs that do not add up to the
 * problem's sample count fail with TWK_HIP_E_INVALID (found on the device: the rows of this call are
 * then undefined). */
typedef struct {
	uint64_t offset;   /* byte offset of the variant's first run word in `bytes` */
	uint32_t n_runs;
	uint8_t  width;    /* bytes per run word: 1, 2 or 4 (twk1_t.gt_ptype)        */
	uint8_t  missing;  /* twk1_t.gt_missing: two bits per allele in the run word */
	uint16_t _pad;
} twk_hip_rle_desc;
int twk_hip_upload_rle(twk_hip_ctx* ctx, uint32_t first, uint32_t count, const void* bytes, size_t n_bytes,
                       const twk_hip_rle_desc* desc, const twk_hip_variant_meta* meta);

/* Read variants [first, first+count) back in the reference layout (twk_igt_vec::data / ::mask,
 * include/core.h:724-753): the inverse of twk_hip_upload_bitvectors, whatever way the rows were put
 * there (bitvectors, run-length words, the synthetic generator).  mask may be NULL; variants without
 * missing genotypes get an all-zero mask.  Parity tests of the device-side T1 use it. */
int twk_hip_download_bitvectors(twk_hip_ctx* ctx, uint32_t first, uint32_t count,
                                uint64_t* data, uint64_t* mask, size_t stride64);

/* Fill the whole problem with the synthetic benchmark input of SURVEY 8(d)
 * directly in HBM (iid alleles, per-variant ALT frequency U(0.05,0.5), one
 * contig, pos = 1000+100*v, no missing data).  Bit-identical to the host
 * generator twk_synth_bitvector() below. */
int twk_hip_generate_synthetic(twk_hip_ctx* ctx, uint64_t seed);
/* The same for a slab: local variant v is global variant first_variant + v (bits, ALT
 * frequency and position all follow the global id), so that ranks that hold different
 * slabs of one synthetic data set agree on every variant they share (halo). */
int twk_hip_generate_synthetic_range(twk_hip_ctx* ctx, uint64_t seed, uint32_t first_variant);
/* Host twin of the device generator: writes variant v's bitvector
 * (ceil(2N/64) words) and returns its ALT allele count. */
uint32_t twk_synth_bitvector(uint64_t seed, uint32_t n_samples, uint32_t v, uint64_t* out_words);

/* The same input with LD planted in it: iid genotypes have no pair near the default r2 cut-off, so a run over them exercises
 * neither the recount of screened-in pairs nor the pair math, Fisher's test, the sort and the way out.  With a plant, odd variant
 * 2k + 1 (k < n_planted; global ids) is a noisy copy of the even variant 2 ((k mult + offset) mod half): every allele of the
 * source flipped with probability eps_k = max_eps u_k, u_k ~ U[0, 1) from the seed.  Sources are never copies, and with mult
 * coprime to half no two copies share a source: the data set then holds exactly n_planted pairs in LD - r2 from 1 down to about
 * (1 - 2 max_eps)^2 - spread over the whole pair triangle (mult large) or at a fixed distance 2 offset - 1 (mult = 1; window
 * runs), and nothing else above r2 ~ 30 / N.  plant == NULL or n_planted == 0: twk_hip_generate_synthetic_range.
 * Constraints (else TWK_HIP_E_INVALID): n_planted <= half, mult >= 1, 0 <= max_eps <= 0.5.  `half` describes the GLOBAL data
 * set (n_variants / 2): the slabs of one data set (first_variant) all pass the same plant and agree on every variant they share.
 * No reference counterpart (the reference's benchmarks read 1000 Genomes files, docs/tutorial.md:177-199). */
typedef struct {
	uint32_t n_planted; /* copies: global variants 1, 3, ..., 2 n_planted - 1                       */
	uint32_t half;      /* sources are the global variants 2 j, j < half                             */
	uint32_t mult;      /* j = (k mult + offset) mod half                                            */
	uint32_t offset;
	double   max_eps;   /* largest flip probability                                                  */
} twk_hip_plant;
int twk_hip_generate_synthetic_planted(twk_hip_ctx* ctx, uint64_t seed, uint32_t first_variant, const twk_hip_plant* plant);
/* Host twins: global variant v of the planted data set (ceil(2N/64) words; returns its ALT allele count), and whether v is a
 * copy (returns 1 and its source / flip probability; 0 and *src = v, *eps = 0 otherwise).  Bit-identical to the device. */
uint32_t twk_synth_planted_bitvector(uint64_t seed, uint32_t n_samples, uint32_t v, const twk_hip_plant* plant, uint64_t* out_words);
int twk_synth_plant_source(uint64_t seed, const twk_hip_plant* plant, uint32_t v, uint32_t* src, double* eps);

/* Copy back per-variant ALT allele count / het / hom-alt / missing-sample
 * counts as seen by the device (popcounts of the planes).  Any pointer may be
 * NULL. */
int twk_hip_get_marginals(twk_hip_ctx* ctx, uint32_t* ac, uint32_t* n_het, uint32_t* n_hom,
                          uint32_t* n_miss_samples);

/* ---- sample subsets ---------------------------------------------------- */
/* LD over a chosen set of samples - one population of a cohort, PLINK's --keep - selected on the device from the data that is already
 * there.  keep: n_keep sample indices into the data AS UPLOADED (the SOURCE), strictly ascending.  After the call the context is a
 * problem of n_keep samples and the same variants, the WORKING SET, and that problem is indistinguishable from a context that received
 * the subset through twk_hip_set_problem + twk_hip_upload_bitvectors: twk_hip_download_bitvectors returns the same data and mask words,
 * padding bits zero; twk_hip_get_marginals and twk_hip_get_meta return the same numbers; every compute entry point returns the same
 * bytes.  Sample k of the working set is source sample keep[k]; variant indices, pos and rid are untouched, and a variant that is
 * monomorphic in the subset stays (the pair rules deal with ac = 0), so that indices stay comparable between subsets.
 * THE SOURCE STAYS ON THE DEVICE: a second call selects from the source again, not from the previous selection - population after
 * population from one upload - and twk_hip_select_samples(ctx, NULL, 0) drops the selection: the context is the source again, bit for
 * bit, without a re-upload.  A list of all the samples is a selection like any other.
 * MEMORY: the working set's rows live beside the source's: M_alloc * Wp' * 4 bytes, twice that while the source holds mask rows, where
 * M_alloc = n_variants rounded up to a multiple of 128, plus 128, and Wp' = ceil(2 n_keep / 32) rounded up to a multiple of 32; the
 * working mask rows are freed again when no working variant has missing data.  During the call 32 bytes per source word with a kept
 * sample (the table) and 8 bytes per variant on top.  TWK_HIP_E_NOMEM with the byte count in twk_hip_last_error.
 * RECOMPUTED ON THE DEVICE for the working set, from its rows: ac[v] = the ALT alleles of the kept samples (popcount of the data row);
 * an[v] = the popcount of the mask row: two per kept sample with a missing genotype; missing[v] = an[v] != 0.  The mask rows are kept
 * only while some working variant is missing, and a variant whose missing samples were all dropped is a variant without missing data:
 * TWK_HIP_MODE_AUTO takes the phased math for it, as it would after a re-import.  `an` equals the importer's count except where a kept
 * sample misses exactly ONE allele: the raw layout marks the whole sample and does not record that case (the importer counts 1, this
 * counts 2), and the device reads `an` only as zero / non-zero.
 * hwe IS LEFT AS UPLOADED: it only sets two flag bits of a record and its exact test lives in the host library; a caller that wants the
 * subset's own Hardy-Weinberg P writes it with twk_hip_set_hwe, which changes the working set only - the next selection, and dropping
 * the selection, bring the uploaded values back.
 * All derived state - contraction planes, sorted plane sets, carrier lists, cached popcounts - is dropped as after an upload and
 * rebuilt on next use; the log-factorial table sized for the source covers every subset.
 * REFUSALS, on each of which nothing changes and a selection that was active stays active: TWK_HIP_E_INVALID for keep == NULL with
 * n_keep != 0, an empty list, a list that is not strictly ascending or holds an index >= the source's sample count (twk_hip_last_error
 * names the position); TWK_HIP_E_STATE before the first upload (or generator call).  WHILE A SELECTION IS ACTIVE twk_hip_upload_bitvectors,
 * twk_hip_upload_rle and the synthetic generators return TWK_HIP_E_STATE: the caller drops it first.  twk_hip_set_problem discards
 * source and selection alike.  A caller that never selects sees no change anywhere.
 * The kernel (csrc/hip/ld_subset.hip.h) reads, per variant, the source words that hold a kept sample - once - and writes the compacted
 * rows with plain stores, every word by one block: two calls give the same bytes.  There is NO reference counterpart (the reference
 * computes over all samples of its input). */
int twk_hip_select_samples(twk_hip_ctx* ctx, const uint32_t* keep, uint32_t n_keep);
/* The sample count of the source and of the working set (either may be NULL); equal when no selection is active (or all are kept). */
int twk_hip_selection(const twk_hip_ctx* ctx, uint32_t* n_source, uint32_t* n_selected);
/* The metadata of variants [first, first + count) of the working set, as the engine holds it: what was uploaded, or what a selection
 * recomputed (ac, an, missing) beside what it left alone (pos, rid, hwe). */
int twk_hip_get_meta(twk_hip_ctx* ctx, uint32_t first, uint32_t count, twk_hip_variant_meta* out);
/* Overwrite the hwe of variants [first, first + count) of the working set. */
int twk_hip_set_hwe(twk_hip_ctx* ctx, uint32_t first, uint32_t count, const double* hwe);
/* Of the context's last selection that ran the kernel: its device time in ms, the bytes of source rows it read (the words with a kept
 * sample, of every variant, data and mask rows) and the bytes of working rows it wrote (any may be NULL). */
int twk_hip_select_last(const twk_hip_ctx* ctx, double* select_ms, uint64_t* bytes_read, uint64_t* bytes_written);

/* ---- variant subsets --------------------------------------------------- */
/* The other axis: LD over the variants that pass a list and frequency / missingness / Hardy-Weinberg thresholds - PLINK's --extract,
 * --exclude, --maf, --max-maf, --mac, --geno and --hwe - decided on the device from the data that is already there.
 * THE BASE is the context as it stands when no variant selection is active: the data as uploaded, or the working set of an active sample
 * selection, its hwe including what twk_hip_set_hwe wrote.  So the order is PLINK's: samples first, then the variants on the kept
 * samples' own counts.
 * THE RULE: variant v of the base is KEPT iff it passes the list and every threshold.  list: n_list base indices, strictly ascending;
 * exclude == 0: v must be in the list, exclude != 0: v must not be; list == NULL with n_list == 0: no list test.  The thresholds are a pure
 * function of what twk_hip_get_marginals and twk_hip_get_meta return for the base: with N the base's sample count, called = N - n_miss,
 * obs = 2 called, alt = n_het + 2 n_hom, minor = min(alt, obs - alt), v passes iff
 *     (double)minor >= min_maf * (double)obs   and   (double)minor <= max_maf * (double)obs   and   minor >= min_mac
 *     and   (double)n_miss <= max_missing * (double)N   and   !(hwe < min_hwe)
 * - each one IEEE double multiplication and one comparison, so equality with a threshold keeps the variant and a NumPy restatement gives
 * the same answer on every input.  filter == NULL: every threshold off (min_maf 0, max_maf 0.5, min_mac 0, max_missing 1, min_hwe 0).
 * THE CONTRACT is the sample subsets': after the call the context is a problem of *n_kept variants and the same samples, in base order,
 * indistinguishable from a context that received exactly those rows and that metadata (the base's hwe included) through
 * twk_hip_set_problem + twk_hip_upload_bitvectors: the downloads, the marginals, the metadata and every compute entry point return the
 * same bytes.  Variant indices everywhere - slices, idxA / idxB, per-variant outputs and per-variant inputs (clump's p, annotations,
 * aggregate's bins) - are WORKING indices 0 .. *n_kept - 1; twk_hip_variant_map gives working -> base.  File order is preserved.  The
 * mask rows are dropped when no kept variant has missing data, and TWK_HIP_MODE_AUTO then takes the phased math, as after a re-import.
 * STATE: a second call selects from the base again ("A then B" equals "B").  twk_hip_select_variants(ctx, NULL, NULL, 0, 0, ..) drops the
 * selection: the context is the base again bit for bit - rows, metadata, an active sample selection.  WHILE A VARIANT SELECTION IS ACTIVE
 * twk_hip_select_samples, the uploads and the generators return TWK_HIP_E_STATE: the caller drops it first.  twk_hip_set_hwe writes the
 * working set only.  twk_hip_set_problem discards everything.
 * MEMORY: THE BASE STAYS ON THE DEVICE, untouched, and the working set lives beside it: M_alloc' * Wp * 4 bytes of rows, twice that while
 * a kept variant has missing data, plus 28 bytes of metadata per row, where M_alloc' = *n_kept rounded up to a multiple of 128, plus 128,
 * and Wp the base's row pitch in words.  During the call 16 bytes per base variant on top (list flags, kept flags, scan, map) and the
 * scan's scratch.  Dropping the selection copies nothing: the base's buffers become the context's again.
 * REFUSALS, on each of which nothing changes and a selection that was active stays active: TWK_HIP_E_INVALID for a list that is not
 * strictly ascending or holds an index >= the base's variant count (twk_hip_last_error names the position), list == NULL with
 * n_list != 0, a threshold that is NaN or outside its range (min_maf, max_maf in [0, 0.5] with min_maf <= max_maf; max_missing, min_hwe
 * in [0, 1]), a selection that keeps no variant; TWK_HIP_E_STATE before the first upload (or generator call); TWK_HIP_E_NOMEM with the
 * byte count.
 * The kernels (csrc/hip/ld_varsel.hip.h): one wave per base variant counts het / hom / missing from its raw rows in one pass and applies
 * the rule; an exclusive scan of the flags gives the map; the rows and the metadata SoA are gathered through it with 16-byte accesses,
 * every output word written once by a plain store, the padding rows as zeros: two calls give the same bytes.  There is NO reference
 * counterpart. */
typedef struct {
    double   min_maf, max_maf;   /* off: 0, 0.5 */
    uint32_t min_mac, _pad;      /* off: 0      */
    double   max_missing;        /* off: 1      */
    double   min_hwe;            /* off: 0      */
} twk_hip_variant_filter;
int twk_hip_select_variants(twk_hip_ctx* ctx, const twk_hip_variant_filter* filter /* NULL: all off */,
                            const uint32_t* list, uint32_t n_list, int32_t exclude, uint32_t* n_kept /* may be NULL */);
/* The variant count of the base and of the working set (either may be NULL); equal when no selection is active (or all are kept). */
int twk_hip_variant_selection(const twk_hip_ctx* ctx, uint32_t* n_before, uint32_t* n_selected);
/* index_before[i] = the base index of working variant first + i (the identity while no selection is active). */
int twk_hip_variant_map(const twk_hip_ctx* ctx, uint32_t first, uint32_t count, uint32_t* index_before);
/* Of the context's last variant selection that ran the kernels: their device time in ms (predicate, scan and map; row and metadata
 * gather), the bytes of rows read (the base's rows once for the predicate, the kept rows once for the gather) and the bytes of working
 * rows written, padding rows included (any may be NULL). */
int twk_hip_select_variants_last(const twk_hip_ctx* ctx, double* select_ms, uint64_t* bytes_read, uint64_t* bytes_written);

/* ---- compute ---------------------------------------------------------- */
/* Raw contingency counts for one tile (debug/parity entry point; replaces the
 * `helper.alleleCounts` filled by the K1-K6 kernels before the math).
 * mode PHASED  : out[4*(i*nB+j)+{0,1,2,3}] = REFREF, ALTREF(1), REFALT(4), ALTALT(5)
 *                cells of twk_ld_count (ld_engine.h:27-30).
 * mode UNPHASED: out[9*(i*nB+j)+k] = cells {0,1+4,5,16+64,17+20+65+68,21+69,80,81+84,85}.
 * Pairs excluded by `diag` are zero-filled. */
int twk_hip_count_tile(twk_hip_ctx* ctx, int mode, const twk_hip_tile_desc* tile, uint64_t* out);

/* LD for one tile: counts -> math -> filters -> compacted survivors.
 * `out` is a HOST buffer of `capacity` records; *n_out receives the number of
 * survivors (on TWK_HIP_E_OVERFLOW: the number required, nothing guaranteed in
 * out).  *n_pairs (may be NULL) receives the number of pairs compared, counted
 * as the reference's progress counter does (ld_engine.cpp:1933,2015). */
int twk_hip_ld_tile(twk_hip_ctx* ctx, int mode, const twk_hip_tile_desc* tile,
                    const twk_hip_filters* filters, twk_hip_record* out, uint64_t capacity,
                    uint64_t* n_out, uint64_t* n_pairs);

/* All-vs-all LD over the upper triangle, restricted to shard `part` of
 * `n_parts`: shard k is the contiguous band of rows that holds the k-th n_parts-th
 * of the pairs (equal-area bands of the triangle, boundaries on multiples of 64
 * variants; every rank derives the same partition without communication).  This
 * replaces twk_ld_balancer::Build (ld_balancing.h:23-80) for multi-GPU sharding.
 * tile_variants = edge of a super-tile in variants (0 = choose: launches sized
 * by their work where no count matrix is kept, see the "band_launch" switch).
 * Survivors are handed to `sink` (may be NULL to discard) launch by launch, one
 * call at a time, all of them before this function returns - launches with
 * many survivors from a second thread of the engine while the calling thread
 * goes on with the launches, the others from the calling thread once that
 * thread has caught up (option "async_delivery", default 1; 0: always the
 * calling thread) -
 * a launch's survivors in pieces of at most 2^20 records; the
 * records of one sink call are in (idxA, idxB) order (sorted on the device), the
 * pieces of a launch follow each other in that order, and a piece stays valid
 * until the sink returns.  *n_pairs / *n_records (may be NULL)
 * receive totals for this shard.
 * The order of the launches is the engine's.  TWK_HIP_MODE_UNPHASED over the whole triangle,
 * without a window, on planes without missing genotypes, with rows too long for the
 * fused form, an r2 cut-off above 1e-6, option "three" = 1 and tile_variants = 0 walks
 * the variants in order of minor allele count (a second, sorted copy of the planes; if it
 * cannot be allocated the call walks the file order): the launches over the rows with few
 * hom-alt carriers then contract two products a pair instead of three (option "two",
 * DESIGN 3.1b).  Every pair is still contracted - no band, no carrier lists - and part /
 * n_parts shard the sorted triangle, the same for every rank; the records are those of the
 * file-order walk, idxA < idxB in file order as always. */
typedef int (*twk_hip_record_sink)(void* user, const twk_hip_record* recs, uint64_t n);
int twk_hip_ld_all(twk_hip_ctx* ctx, int mode, const twk_hip_filters* filters,
                   uint32_t part, uint32_t n_parts, uint32_t tile_variants,
                   int32_t window, uint32_t l_window,
                   twk_hip_record_sink sink, void* user, uint64_t* n_pairs, uint64_t* n_records);

/* Same over a sub-region of the pair space: rows [a0,a0+nA) x cols [b0,b0+nB).
 * triangle != 0 (requires a0 == b0, nA == nB): only col > row.  This is what a
 * `-c/-C` chunk of the reference is (ld_balancing.h:59-78: diagonal or square). */
int twk_hip_ld_region(twk_hip_ctx* ctx, int mode, const twk_hip_filters* filters,
                      uint32_t a0, uint32_t nA, uint32_t b0, uint32_t nB, int32_t triangle,
                      uint32_t part, uint32_t n_parts, uint32_t tile_variants,
                      int32_t window, uint32_t l_window,
                      twk_hip_record_sink sink, void* user, uint64_t* n_pairs, uint64_t* n_records);

/* LD scores over the same slice of the pair space, with the same arguments: for every variant v of the problem
 *   n_partners[v] = the number of records twk_hip_ld_region would report with v as idxA or idxB,
 *   sum_r2[v]     = the sum of their R2 fields
 * - with filters.minR2 = 0 the LD score of v, with minR2 = 0.8 its number of tagging partners - reduced on the device:
 * the count matrix of a launch goes through the pair rules and the math of the record path (skips, the default mode's
 * per-pair choice of math, D = 0, the cubic's roots, window, r2 / D' bounds, option bits: one code, ld_math.hip.h) and the
 * r2 of the pairs that survive is summed per row and per column (ld_score.hip.h).  No record is formed, sorted or copied:
 * 16 bytes per variant leave the device.  filters.minP must be >= 1 (TWK_HIP_E_INVALID otherwise): the two-sided P never
 * exceeds 1, so that bound drops nothing and Fisher's test is not run.  Always the matrix form of the contraction (no r2
 * band, no fused screen, no carrier lists: a score looks at every pair; TWK_HIP_OPT_R2_SCREEN is ignored).  n_partners /
 * sum_r2: HOST arrays of n_variants entries each, indexed by variant as uploaded, overwritten (variants outside the slice:
 * 0 / 0.0).  A shard (part / n_parts: the rows of twk_hip_ld_region's shard) returns partial arrays over all variants; the
 * shards' arrays add up to the whole.  The sums are formed in a fixed order without floating-point atomics: two calls with
 * the same arguments return the same bits.  *n_pairs (may be NULL): pairs evaluated.  twk_hip_timing: the score kernels
 * count as the math stage (stats_ms, stats_launches, variant_pairs).  There is NO reference counterpart: the reference
 * writes records only, and a score is a sum over its output file. */
int twk_hip_ld_score(twk_hip_ctx* ctx, int mode, const twk_hip_filters* filters,
                     uint32_t a0, uint32_t nA, uint32_t b0, uint32_t nB, int32_t triangle,
                     uint32_t part, uint32_t n_parts, uint32_t tile_variants,
                     int32_t window, uint32_t l_window,
                     uint64_t* n_partners, double* sum_r2, uint64_t* n_pairs);

/* LD pruning (PLINK's --indep-pairwise, greedy in file order) of the contiguous triangle of variants [a0, a0 + n), with the mode,
 * filters, tile_variants, window bits and l_window of twk_hip_ld_region:
 *   a pair (u, v), u < v, is an EDGE if twk_hip_ld_region over that triangle would report a record with those two variants;
 *   walking v = a0 .. a0 + n - 1 upwards, v is KEPT if and only if no kept u < v has an edge (u, v).
 * A variant the pair rules never report (the low-allele-count rule, say) has no edge and is kept.  Decided on the device: the count
 * matrix of a launch goes through the pair rules and the math of the record path (one code, ld_math.hip.h), `keep` of every pair is
 * balloted into an adjacency bitmap, and one sequential kernel walks the bitmap (ld_prune.hip.h).  No record is formed, sorted or
 * copied: one byte per variant leaves the device.
 *   keep     HOST array of n_variants bytes, indexed by variant as uploaded, overwritten: 1 kept, 0 dropped or outside the slice
 *   *n_kept  (may be NULL) the number of 1s;  *n_edges (may be NULL) the number of records twk_hip_ld_region would have reported;
 *   *n_pairs (may be NULL) pairs evaluated.
 * The result is a function of the edge set alone and bitwise OR has no order: two calls with the same arguments return the same bytes.
 * Always the whole triangle on one device (the walk needs every edge: there is no part / n_parts and no rectangle here), always the
 * matrix form of the contraction (TWK_HIP_OPT_R2_SCREEN is ignored, as for a score).  filters.minP must be >= 1 (TWK_HIP_E_INVALID
 * otherwise, before any launch): Fisher's test is not run.  Device memory: n * ceil(n / 64) * 8 bytes for the bitmap for the length of
 * the call (0.31 GB at 50,000 variants, 35 GB at 531,500), whatever the window; TWK_HIP_E_NOMEM with the size in twk_hip_last_error
 * when the device cannot give it.  twk_hip_timing: the mask kernels count as the math stage (stats_ms, stats_launches,
 * variant_pairs); the walk is reported by twk_hip_prune_last.  There is NO reference counterpart. */
int twk_hip_ld_prune(twk_hip_ctx* ctx, int mode, const twk_hip_filters* filters, uint32_t a0, uint32_t n, uint32_t tile_variants,
                     int32_t window, uint32_t l_window, uint8_t* keep, uint64_t* n_kept, uint64_t* n_edges, uint64_t* n_pairs);
/* Of the context's last twk_hip_ld_prune call: the device time of its walk kernel in ms and the size of its bitmap (either may be NULL). */
int twk_hip_prune_last(const twk_hip_ctx* ctx, double* walk_ms, uint64_t* bitmap_bytes);

/* LD clumping (PLINK's --clump) of the triangle of variants [a0, a0 + n) in file order, without records.  mode, filters, tile_variants,
 * window (the option bits) and l_window are those of twk_hip_ld_region.
 *   {u, v} is an EDGE if twk_hip_ld_region over that triangle would report a record with those two variants (prune's edge, seen from
 *   both ends);  v is ELIGIBLE if p[v] is not NaN and p[v] <= p2;
 *   the variants of the slice whose p is not NaN are visited in ascending p, ties in file order, up to the first with p > p1.  A visited
 *   variant that already belongs to a clump is skipped; otherwise it becomes an INDEX variant, index_of[v] = v, and every eligible w
 *   with an edge to v that belongs to no clump yet gets index_of[w] = v.
 * Decided on the device: `keep` of every pair of a launch's count matrix - the pair rules and the math of the record path, one code
 * (ld_math.hip.h) - is set in an adjacency bitmap at (u, v) and at (v, u), and one sequential kernel walks the bitmap in P order
 * (ld_clump.hip.h).  No record is formed, sorted or copied: four bytes per variant leave the device.
 *   p          HOST array of n_variants doubles, indexed by variant as uploaded: the association P value, NaN for none
 *   p1, p2     the index and the secondary threshold, 0 <= p1 <= p2 <= 1
 *   index_of   HOST array of n_variants uint32, overwritten: the variant's index variant (itself for an index variant), or
 *              TWK_HIP_NO_CLUMP - unclaimed, no P value, or outside the slice
 *   *n_clumps  (may be NULL) the number of index variants;  *n_members (may be NULL) the number of claimed variants that are not
 *   index variants;  *n_edges (may be NULL) the records twk_hip_ld_region would have reported, each pair once;  *n_pairs (may be NULL)
 * The result is a function of the edge set and p alone: two calls return the same bytes.  With p increasing in file order and
 * p1 = p2 = 1 the index variants are exactly twk_hip_ld_prune's kept set.
 * TWK_HIP_E_INVALID before any launch: filters->minP < 1 (Fisher's test is not run), p or index_of NULL, a threshold that is NaN, out
 * of order or outside [0, 1], a non-NaN p[v] of the slice outside [0, 1], n == 0 or a slice that reaches beyond the last variant.
 * Device memory: n * ceil(n / 64) * 8 bytes for the bitmap for the length of the call, as for twk_hip_ld_prune (the mirrored bits
 * take the half prune leaves empty); TWK_HIP_E_NOMEM with the size in twk_hip_last_error when the device cannot give it.
 * twk_hip_timing: the mask kernels count as the math stage (stats_ms, stats_launches, variant_pairs); the walk is reported by
 * twk_hip_clump_last.  There is NO reference counterpart. */
#define TWK_HIP_NO_CLUMP 0xFFFFFFFFu
int twk_hip_ld_clump(twk_hip_ctx* ctx, int mode, const twk_hip_filters* filters, uint32_t a0, uint32_t n, uint32_t tile_variants,
                     int32_t window, uint32_t l_window, const double* p, double p1, double p2,
                     uint32_t* index_of, uint64_t* n_clumps, uint64_t* n_members, uint64_t* n_edges, uint64_t* n_pairs);
/* Of the context's last twk_hip_ld_clump call: the device time of its walk kernel in ms and the size of its bitmap (either may be NULL). */
int twk_hip_clump_last(const twk_hip_ctx* ctx, double* walk_ms, uint64_t* bitmap_bytes);

/* The dense LD matrix of the triangle of variants [a0, a0 + n) in file order, without records: the input of fine-mapping and of
 * Bayesian polygenic scores.  mode, filters, tile_variants, window (the option bits) and l_window are those of twk_hip_ld_region.
 *   stat   TWK_HIP_STAT_R: copysign(rec.R, rec.D) - the record's R is sqrt(R2) and never negative, the matrix's r carries D's sign;
 *          TWK_HIP_STAT_R2: rec.R2;  TWK_HIP_STAT_D: rec.D;  TWK_HIP_STAT_DPRIME: rec.Dprime
 *   out    HOST array of n rows of ld >= n floats.  For u != v relative to a0: if twk_hip_ld_region over that triangle would report a
 *          record for the two variants, out[u * ld + v] is that record's statistic, computed in double and rounded once to float32
 *          ((float)x, to nearest); otherwise it is `fill`, bit for bit (any pattern, NaN included) - the low-allele-count skip,
 *          D == 0, outside the window, below a cut-off.  All four statistics are symmetric in the two variants: out[u * ld + v] and
 *          out[v * ld + u] hold the same bits.  With fill = 0 and minR2 = 0 this is the matrix a fine-mapper expects; with minR2 > 0
 *          the sparsified one.
 *          THE DIAGONAL is 1.0f for R, R2 and DPRIME, whatever the variant's allele count, and `fill` for D: no record pins a
 *          variant's variance under missing data, and the function invents none.
 *          The columns n .. ld - 1 of every row are not written.
 *   *n_records  (may be NULL) the off-diagonal pairs that received a value, each pair once: the records `calc` would have written;
 *   *n_pairs    (may be NULL) the pairs evaluated.
 * Always the whole triangle on one device and always the matrix form of the contraction: TWK_HIP_OPT_R2_SCREEN is ignored, as for a
 * score; there is no part / n_parts and no rectangle.  Every entry is written by plain stores, by exactly one lane of exactly one
 * launch (in the default mode the two passes select disjoint pairs) or by the preset: no atomics, two calls return the same bytes.
 * TWK_HIP_E_INVALID before any launch: minP < 1, out NULL, ld < n, n == 0, a slice beyond the last variant, an unknown stat.
 * Device memory: n * n * 4 bytes for the length of the call; TWK_HIP_E_NOMEM with the size in twk_hip_last_error when the device
 * cannot give it.  The matrix leaves the device in one 2-D copy that honours ld.
 * twk_hip_timing: the fill kernels count as the math stage (stats_ms, stats_launches, variant_pairs); the copy is reported by
 * twk_hip_matrix_last.  There is NO reference counterpart. */
enum { TWK_HIP_STAT_R = 0, TWK_HIP_STAT_R2 = 1, TWK_HIP_STAT_D = 2, TWK_HIP_STAT_DPRIME = 3 };
int twk_hip_ld_matrix(twk_hip_ctx* ctx, int mode, const twk_hip_filters* filters,
                      uint32_t a0, uint32_t n, uint32_t tile_variants, int32_t window, uint32_t l_window,
                      int32_t stat, float fill, float* out, uint64_t ld,
                      uint64_t* n_records, uint64_t* n_pairs);
/* Of the context's last twk_hip_ld_matrix call: the time of its device-to-host copy in ms and the matrix's bytes (either may be NULL). */
int twk_hip_matrix_last(const twk_hip_ctx* ctx, double* copy_ms, uint64_t* matrix_bytes);

/* The banded LD matrix: twk_hip_ld_matrix's values of a WINDOWED run in band storage - per row only the columns inside the window - so
 * that a chromosome-wide LD reference panel (what LDpred2, PRS-CS, SBayesR and summary-statistics imputation read) fits where the dense
 * n * n * 4 bytes do not.  The variants of the slice [a0, a0 + n) must be sorted by (rid, pos), as in every .twk.
 * THE LAYOUT, for a window of l_window base pairs: the band of row u is the contiguous column range [first[u], first[u] + len[u]),
 * relative to the slice: the variants v of the slice on u's contig with |pos[u] - pos[v]| <= l_window - exactly the rule of the window
 * test of twk_hip_ld_region.  It is symmetric, includes the diagonal, and is clipped at contig and slice borders.  row_ptr[u] is the sum
 * of len[0 .. u), row_ptr[n] the number of stored floats; len[u] = row_ptr[u + 1] - row_ptr[u].
 *   twk_hip_bandmat_layout  first (HOST, n entries) and row_ptr (HOST, n + 1 entries) from the uploaded metadata, on the host, so that
 *          a caller can size `values`.  TWK_HIP_E_INVALID: a NULL argument, n == 0, a slice beyond the last variant, a slice that is not
 *          sorted by (rid, pos); TWK_HIP_E_STATE before upload.
 *   twk_hip_ld_matrix_band  mode, filters, a0, n, tile_variants, l_window, stat, fill, n_records and n_pairs are twk_hip_ld_matrix's;
 *          `window` holds the option bits and TWK_HIP_OPT_WINDOW must be set.
 *          values  HOST array of `capacity` >= row_ptr[n] floats.  For every in-band (u, v), values[row_ptr[u] + (v - first[u])] holds,
 *                  bit for bit, what twk_hip_ld_matrix with the same arguments puts in out[u * n + v]: the statistic rounded once to
 *                  float32 where twk_hip_ld_region would report a record, `fill` where it would not, and on the diagonal 1.0f for R,
 *                  R2 and DPRIME and `fill` for D.  Nothing beyond values[row_ptr[n] - 1] is written.  Both orientations are stored:
 *                  (values, the columns first[u] .. first[u] + len[u] - 1 of every row, row_ptr) is a CSR matrix as it stands.
 *          first, row_ptr  HOST arrays of n and n + 1 entries, overwritten with the layout.
 *          TWK_HIP_E_INVALID before any launch, with nothing written to values, first or row_ptr: twk_hip_ld_matrix's own refusals
 *          (minP < 1, n == 0, a slice beyond the last variant, an unknown stat), TWK_HIP_OPT_WINDOW not set, a NULL values, first or
 *          row_ptr, capacity < row_ptr[n], a slice that is not sorted.  Device memory: row_ptr[n] * 4 + n * 16 bytes for the length of
 *          the call; TWK_HIP_E_NOMEM with the byte count in twk_hip_last_error when the device cannot give it.  Plain stores, every
 *          entry by exactly one lane of one launch or by the preset: two calls return the same bytes, whatever tile_variants.  The band
 *          leaves the device in one contiguous copy.  twk_hip_timing: the fill kernels count as the math stage.
 *   twk_hip_bandmat_last  of the context's last twk_hip_ld_matrix_band call: the time of its device-to-host copy in ms and the band's
 *          bytes, row_ptr[n] * 4 (either may be NULL).
 * There is NO reference counterpart. */
int twk_hip_bandmat_layout(twk_hip_ctx* ctx, uint32_t a0, uint32_t n, uint32_t l_window, uint32_t* first, uint64_t* row_ptr);
int twk_hip_ld_matrix_band(twk_hip_ctx* ctx, int mode, const twk_hip_filters* filters,
                           uint32_t a0, uint32_t n, uint32_t tile_variants, int32_t window, uint32_t l_window,
                           int32_t stat, float fill, float* values, uint64_t capacity, uint32_t* first, uint64_t* row_ptr,
                           uint64_t* n_records, uint64_t* n_pairs);
int twk_hip_bandmat_last(const twk_hip_ctx* ctx, double* copy_ms, uint64_t* band_bytes);

/* Haplotype blocks by the rule of Gabriel et al. (2002) - PLINK's --blocks, Haploview's default view - in two calls, one on top of the
 * other.  Both are windowed (l_window base pairs, always on), both take twk_hip_ld_matrix_band's mode, filters (minP >= 1), a0, n and
 * tile_variants, and an INFORMATIVE pair is one for which twk_hip_ld_region with the same arguments would report a record.
 *   twk_hip_ld_dprime_ci_band  the confidence bounds of D' of every informative in-band pair, in twk_hip_bandmat_layout's layout for
 *          l_window: lo and hi, HOST arrays of `capacity` >= row_ptr[n] bytes each, hold at row_ptr[u] + (v - first[u]) the bounds of
 *          the pair (u, v) in percent, 0 .. 100 - both orientations - and 255 / 255 where the pair has no record, and on the diagonal.
 *          The bounds are those of a likelihood scan over 101 values of D' of the record's 2 x 2 table cnt[0..3]: the lowest and the
 *          highest grid point that leave 5 % of the likelihood's mass outside, one step outwards (DESIGN 3.18 has the definition to the
 *          rounding).  first, row_ptr: overwritten with the layout.  n_records: the informative pairs u < v.  Refusals: as
 *          twk_hip_ld_matrix_band's, and l_window == 0.  Plain stores, no atomics: the same bytes for any tiling and on any repeat.
 *   twk_hip_ld_blocks  the blocks of the slice's variants in file order.  params: NULL for the defaults
 *          {70, 98, 90, 80, 50, 950, 20000, 30000}.  l_window is also the longest block in base pairs.
 *          A CANDIDATE is an informative pair i < j with lo >= strong_lo and hi >= strong_hi; m = j - i + 1 is its marker count and
 *          sep = pos[j] - pos[i].  Its cut-off is strong_lo_2 for m = 2, strong_lo_34 for m = 3 or 4, strong_lo otherwise.  Over the
 *          informative pairs x < y inside [i, j], s counts those with lo >= cut && hi >= strong_hi and r those with hi < recomb_hi.
 *          It QUALIFIES iff not (m == 2 && sep > max_span_2), not (m == 3 && sep > max_span_3), s + r >= 1 (m = 2), 3 (m = 3) or
 *          6 (m >= 4), and s * 1000 > inform_permille * (s + r).  The qualifying candidates are visited in order of sep descending,
 *          then m descending, then i ascending; one becomes a BLOCK iff neither of its ends lies in an earlier block.
 *          block_of  HOST, one entry per uploaded variant: the index of the first variant of the variant's block, or TWK_HIP_NO_BLOCK
 *                    (also outside the slice).
 *          first, last, n_strong, n_recomb  HOST arrays of n / 2 entries (each may be NULL): per block, in file order, its first and
 *                    last variant and its s and r.
 *          n_blocks, n_candidates, n_informative, n_pairs  (each may be NULL) blocks, candidates, informative pairs, pairs looked at.
 *          TWK_HIP_E_INVALID before any launch: a threshold above 100, recomb_hi > strong_hi, inform_permille > 1000, minP < 1,
 *          l_window == 0, n == 0, a slice beyond the last variant or not sorted, a NULL block_of, a band row wider than 65,535
 *          variants, a sort key (window, widest row, n) beyond 64 bits.  Device memory for the length of the call: 10 bytes per band
 *          slot and 32 per qualifying candidate; TWK_HIP_E_NOMEM with the byte count in twk_hip_last_error.  The result is a function
 *          of the lo / hi bytes, the positions and the parameters alone.
 *   twk_hip_blocks_last  of the context's last twk_hip_ld_blocks call: the walk kernel's time in ms and the bytes of the lo / hi band
 *          (either may be NULL).
 * There is NO reference counterpart; PLINK and Haploview add a LOD filter, their own MAF rule and, unphased, a double-heterozygote term. */
#define TWK_HIP_NO_BLOCK 0xFFFFFFFFu
typedef struct twk_hip_block_params {
	uint32_t strong_lo, strong_hi, recomb_hi, strong_lo_2, strong_lo_34, inform_permille, max_span_2, max_span_3;
} twk_hip_block_params;
int twk_hip_ld_dprime_ci_band(twk_hip_ctx* ctx, int mode, const twk_hip_filters* filters,
                              uint32_t a0, uint32_t n, uint32_t tile_variants, uint32_t l_window,
                              uint8_t* lo, uint8_t* hi, uint64_t capacity, uint32_t* first, uint64_t* row_ptr,
                              uint64_t* n_records, uint64_t* n_pairs);
int twk_hip_ld_blocks(twk_hip_ctx* ctx, int mode, const twk_hip_filters* filters,
                      uint32_t a0, uint32_t n, uint32_t tile_variants, uint32_t l_window, const twk_hip_block_params* params,
                      uint32_t* block_of, uint32_t* first, uint32_t* last, uint32_t* n_strong, uint32_t* n_recomb,
                      uint64_t* n_blocks, uint64_t* n_candidates, uint64_t* n_informative, uint64_t* n_pairs);
int twk_hip_blocks_last(const twk_hip_ctx* ctx, double* walk_ms, uint64_t* band_bytes);
/* ... and the device time in ms of its stages between the bounds' launches and the walk: the prefix counts, the counting pass over the
 * candidates and the scan; the emitting pass; the sort (each may be NULL; 0 for a stage that did not run). */
int twk_hip_blocks_stages(const twk_hip_ctx* ctx, double* counts_ms, double* emit_ms, double* sort_ms);

/* LD splitting (Prive 2021, "Optimal linkage disequilibrium splitting"; bigsnpr's snp_ldsplit): where to cut a contig into K blocks of
 * min_size .. max_size variants so that as little r2 as possible crosses a cut, for every K = 1 .. k_max, solved on the device over the
 * banded r2 matrix, which never leaves it.
 *   INPUT    the slice [a0, a0 + n) of the working set, sorted by position on ONE contig; mode, filters (minP >= 1), tile_variants and
 *            l_window > 0 base pairs as for twk_hip_ld_matrix_band; min_size, max_size and k_max in variants.
 *   THE BAND B: what twk_hip_ld_matrix_band with the same arguments, TWK_HIP_STAT_R2 and fill 0.0f writes.
 *   WEIGHTS  for u < v (relative to the slice): q(u, v) = llrint((double)B[u][v] * 2^32) if v lies in u's band, else 0.  The product is
 *            exact in double.  The diagonal is ignored.
 *   OBJECTIVE  within(a, b) = the sum of q(u, v) over a <= u < v < b; T = within(0, n).  A K-partition is 0 = c_0 < c_1 < .. < c_K = n
 *            with min_size <= c_i - c_(i-1) <= max_size; gain_K is the maximum over K-partitions of the sum of within(c_(i-1), c_i), and
 *            cost_K = T - gain_K: the sum of r2 outside the blocks, in units of 2^-32.
 *   RECURRENCE  G_0(0) = 0, G_0(b > 0) infeasible; G_k(b) = the maximum over d in [min_size, min(max_size, b)] with G_(k-1)(b - d)
 *            feasible of G_(k-1)(b - d) + within(b - d, b); D_k(b) is the SMALLEST d that attains it.  The partition reported for K is
 *            the one backtracked from (K, n) through D: among the optimal ones that whose size sequence, read from the last block, is
 *            lexicographically smallest.  64-bit integers throughout: the result is a function of the band's bytes and the three sizes
 *            alone, the same for any tile_variants and on any repeat.
 *   OUTPUT   HOST arrays.  total[0] = T.  feasible[K - 1] (k_max bytes): 1 where a K-partition exists, else 0.  Where it is 1:
 *            cost[K - 1] (k_max entries) = cost_K and cuts[(K - 1) * (k_max + 1) + i] = c_i for i = 0 .. K (k_max * (k_max + 1) entries,
 *            relative to the slice); the entries of cost and cuts of an infeasible K, and beyond c_K in a row, are left untouched.
 *            n_records, n_pairs (each may be NULL): as twk_hip_ld_matrix_band's.
 *   TWK_HIP_E_INVALID before any launch, with nothing written: twk_hip_ld_matrix_band's own refusals, l_window == 0, a slice on two
 *            contigs, min_size == 0, min_size > max_size, max_size > 65535 (D is uint16), k_max == 0 or k_max > 1024,
 *            (uint64_t)n * max_size >= 2^32 (below it every sum of a partition stays under 2^63: at most n * max_size / 2 in-block
 *            pairs of at most 2^32 each), 2^31 or more in-band pairs (T stays under 2^63), a NULL total, feasible, cost or cuts.
 *   DEVICE MEMORY for the length of the call: the band (4 bytes a slot, 16 a variant), 8 bytes per (variant, offset <= min(widest upper
 *            band, max_size - 1)) of row prefixes, 8 per (variant, d in [min_size, max_size]) of block sums - at most 16 bytes per
 *            (variant, d <= max_size) together - 2 * k_max bytes a variant of D and 28 a variant besides;
 *            TWK_HIP_E_NOMEM with the byte count in twk_hip_last_error.
 *   twk_hip_split_last  of the context's last twk_hip_ld_split call: the device time in ms of the band's launches, of row prefixes +
 *            block sums, of the layers and of the backtrack, and the bytes of device memory held (each may be NULL).
 * NOT bigsnpr's max_r2 constraint (no cut is refused for a large r2 across it) and NOT LDetect's filtered-minimum rule.  There is NO
 * reference counterpart. */
int twk_hip_ld_split(twk_hip_ctx* ctx, int mode, const twk_hip_filters* filters,
                     uint32_t a0, uint32_t n, uint32_t tile_variants, uint32_t l_window,
                     uint32_t min_size, uint32_t max_size, uint32_t k_max,
                     uint64_t* total, uint8_t* feasible, uint64_t* cost, uint32_t* cuts, uint64_t* n_records, uint64_t* n_pairs);
int twk_hip_split_last(const twk_hip_ctx* ctx, double* band_ms, double* sums_ms, double* layers_ms, double* backtrack_ms, uint64_t* bytes);

/* LD decay over the same slice of the pair space as twk_hip_ld_score, with the same arguments: r2 as a function of the distance
 * between two variants.  A pair COUNTS when twk_hip_ld_region with these arguments would report a record for it, both variants lie on
 * the same contig and their positions differ; its distance is d = |posA - posB| (on a position-sorted file the reference's rule,
 * ridA == ridB && Apos < Bpos: two_reader::Decay).  With width = range_bp / n_bins (integer division) its bin is
 * min(d / width, n_bins - 1): the last bin also collects everything beyond the range, as in the reference.  For every bin
 *   n[bin]      = the number of counting pairs,
 *   sum_r2[bin] = the sum of their R2 fields
 * (the mean is the caller's division) - reduced on the device: the count matrix of a launch goes through the pair rules and the
 * math of the record path (one code, ld_math.hip.h) and the r2 of a counting pair is added to its bin as the integer
 * rint(r2 * 2^32) (ld_decay.hip.h, ld_exact_sum.h).  No record is formed, sorted or copied: 24 bytes per bin leave the device.
 * THE SUMS ARE EXACT IN INTEGERS AND HAVE NO ORDER: sum_r2[bin] is the sum of the pairs' r2, each rounded once to a multiple of
 * 2^-32 (off by at most 2^-33 a pair), converted to double once; two calls, any tile_variants and any launch order return the same
 * bits, and no floating-point atomic is used.  filters.minP must be >= 1: Fisher's test is not run.  Always the matrix form of the
 * contraction (TWK_HIP_OPT_R2_SCREEN is ignored, as for a score).  n / sum_r2: HOST arrays of n_bins entries each, overwritten.  A
 * shard (part / n_parts) returns partial arrays; the shards' n add up exactly, their sums to within double rounding.
 * *n_pairs (may be NULL): pairs evaluated.
 * TWK_HIP_E_INVALID before any launch: minP < 1, n or sum_r2 NULL, n_bins == 0 or n_bins > 4096 (the block's histogram lives in
 * LDS), range_bp < n_bins (a width of 0), and the region call's own argument errors; TWK_HIP_E_STATE before upload.  A call of more
 * than 2^32 kernel blocks - at least 2^32 blocks of up to 8192 pairs: beyond the accumulators' proven room - ends with
 * TWK_HIP_E_INVALID at the launch that would pass it.  twk_hip_timing: the decay kernels count as the math stage (stats_ms,
 * stats_launches, variant_pairs).  The reference's counterpart bins the records of a sorted .two file on the host. */
int twk_hip_ld_decay(twk_hip_ctx* ctx, int mode, const twk_hip_filters* filters,
                     uint32_t a0, uint32_t nA, uint32_t b0, uint32_t nB, int32_t triangle,
                     uint32_t part, uint32_t n_parts, uint32_t tile_variants,
                     int32_t window, uint32_t l_window,
                     uint32_t range_bp, uint32_t n_bins,
                     uint64_t* n /*[n_bins]*/, double* sum_r2 /*[n_bins]*/, uint64_t* n_pairs);

/* LD aggregate over the same slice of the pair space as twk_hip_ld_score, with the same arguments: the pairwise LD of a region
 * rasterised into x_bins * y_bins cells (the reference's two_reader::Aggregate reads the records of a .two file; here no record is
 * formed).  stat: TWK_HIP_STAT_R (signed: copysign(R, D), as in twk_hip_ld_matrix), _R2, _D or _DPRIME - the pair's value v.
 * bin_x / bin_y: HOST arrays of n_variants uint16_t, indexed by variant as uploaded: the variant's bin on that axis, 0xFFFF for a
 * variant that is off the landscape on it.  The engine never sees positions: what a bin is - a stretch of bases, of genetic distance,
 * an allele-frequency class - is the caller's.  For every pair (A, B) for which twk_hip_ld_region with these arguments would report a
 * record, v is added to cell (bin_x[A], bin_y[B]) and to cell (bin_x[B], bin_y[A]), each orientation if both of its bins are valid
 * (the reference's writer emits every record in both orientations and its aggregator indexes mat[x(A)][y(B)]; when both land in one
 * cell its n grows by 2; no same-contig and no distinct-position rule, as in the reference).  HOST arrays of x_bins * y_bins entries
 * each, cell (x, y) at x * y_bins + y, overwritten:
 *   n       contributions to the cell
 *   sum     the sum of q / 2^32 over the cell, q = rint(v * 2^32) as a signed 64-bit integer
 *   sum_sq  the same with q2 = rint((v * v) * 2^32) - the square is one double multiplication
 *   min/max the smallest and the largest q / 2^32; both 0.0 where n == 0
 * THE SUMS ARE EXACT IN INTEGERS AND HAVE NO ORDER (ld_aggregate.hip.h, ld_exact_sum.h): summed in 64-bit integer atomics,
 * converted once from 128 bits; all five arrays are the same bits for any tile_variants, any launch order and any repeat, and no
 * floating-point atomic is used.  A shard (part / n_parts) returns partial arrays: n and the sums add, min / max combine by min /
 * max over the cells with n != 0.  filters.minP must be >= 1: Fisher's test is not run.  Always the matrix form of the contraction
 * (TWK_HIP_OPT_R2_SCREEN is ignored, as for a score).  *n_pairs (may be NULL): pairs evaluated.  64 bytes of device memory a cell
 * for the length of the call.
 * TWK_HIP_E_INVALID before any launch: minP < 1, a NULL array, x_bins or y_bins 0 or above 4096, a bin entry >= its axis' count
 * that is not 0xFFFF, an unknown stat, and the region call's own argument errors; TWK_HIP_E_STATE before upload.  A call whose
 * launches can evaluate more than 2^42 pairs - beyond the accumulators' proven room - ends with TWK_HIP_E_INVALID at the launch that
 * would pass it.  twk_hip_timing: the aggregate kernels count as the math stage (stats_ms, stats_launches, variant_pairs). */
int twk_hip_ld_aggregate(twk_hip_ctx* ctx, int mode, const twk_hip_filters* filters,
                         uint32_t a0, uint32_t nA, uint32_t b0, uint32_t nB, int32_t triangle,
                         uint32_t part, uint32_t n_parts, uint32_t tile_variants,
                         int32_t window, uint32_t l_window,
                         int32_t stat, const uint16_t* bin_x /*[n_variants]*/, const uint16_t* bin_y /*[n_variants]*/,
                         uint32_t x_bins, uint32_t y_bins,
                         uint64_t* n, double* sum, double* sum_sq, double* min, double* max /*[x_bins * y_bins] each*/, uint64_t* n_pairs);

/* Partitioned LD scores over the same slice of the pair space as twk_hip_ld_score, with the same arguments and the same pair set: what
 * stratified LD-score regression reads, l(v, c) = the sum over v's partners w of a[w][c] * r2(v, w).  annot: HOST array of n_variants
 * rows of ld_annot >= n_annot doubles, indexed by variant as uploaded - binary categories, real-valued ones, anything finite with
 * |a| <= TWK_HIP_ANNOT_MAX_ABS.  A pair COUNTS exactly when twk_hip_ld_region with these arguments would report a record for it.  For
 * each counting pair (A, B) and each category c the integer rint((R2 * a[B][c]) * 2^32) is added to (A, c) and the integer
 * rint((R2 * a[A][c]) * 2^32) to (B, c): one double multiplication, an exact scaling, rounding to nearest with ties to even.
 *   score       HOST array of n_variants * n_annot doubles, row v at v * n_annot, overwritten: the exact integer sum of (v, c),
 *               converted to double once and divided by 2^32
 *   n_partners  HOST array of n_variants entries, overwritten: twk_hip_ld_score's count
 * An annotation of 0 (or -0.0) adds nothing; an annotation of 1 adds rint(R2 * 2^32), the quantum of twk_hip_ld_decay; variants
 * outside the slice get 0.  THE VARIANT ITSELF IS NOT A PARTNER, as in twk_hip_ld_score: a caller that wants LDSC's convention
 * (r2(v, v) = 1) adds a[v][c].
 * THE SUMS ARE EXACT IN INTEGERS AND HAVE NO ORDER (ld_score_annot.hip.h, ld_annot_term.h, ld_exact_sum.h): summed in 64-bit integer
 * atomics, converted once from 128 bits; the same bits for any tile_variants, any launch order and any repeat, and no floating-point
 * atomic is used.  A shard (part / n_parts) returns partial arrays: n_partners adds exactly, the scores to within double rounding.
 * filters.minP must be >= 1: Fisher's test is not run.  Always the matrix form of the contraction (TWK_HIP_OPT_R2_SCREEN is ignored, as
 * for a score).  *n_pairs (may be NULL): pairs evaluated.  The context is left as it was.
 * TWK_HIP_E_INVALID before any launch: minP < 1, a NULL array, n_annot == 0 or above TWK_HIP_ANNOT_MAX_CATEGORIES, ld_annot < n_annot,
 * an annotation of any variant of the problem that is not finite or beyond TWK_HIP_ANNOT_MAX_ABS in magnitude (twk_hip_last_error
 * names the variant and the column), and the region call's own argument errors; TWK_HIP_E_STATE before upload.  Device memory:
 * 24 bytes per variant and category for the length of the call; TWK_HIP_E_NOMEM with the size in twk_hip_last_error when the device
 * cannot give it.  twk_hip_timing: the kernels count as the math stage (stats_ms, stats_launches, variant_pairs).  There is NO
 * reference counterpart. */
#define TWK_HIP_ANNOT_MAX_CATEGORIES 256
#define TWK_HIP_ANNOT_MAX_ABS 65536.0     /* 2^16 */
int twk_hip_ld_score_annot(twk_hip_ctx* ctx, int mode, const twk_hip_filters* filters,
                           uint32_t a0, uint32_t nA, uint32_t b0, uint32_t nB, int32_t triangle,
                           uint32_t part, uint32_t n_parts, uint32_t tile_variants,
                           int32_t window, uint32_t l_window,
                           const double* annot, uint32_t n_annot, uint64_t ld_annot,
                           uint64_t* n_partners /*[n_variants]*/, double* score /*[n_variants * n_annot], row v at v * n_annot*/,
                           uint64_t* n_pairs);

/* Top-k LD partners over the same slice of the pair space as twk_hip_ld_score, with the same arguments and the same pair set: for every
 * variant its k strongest proxies - what LDlink's LDproxy, PLINK's --show-tags and --ld-snp, and proxy substitution for a variant missing
 * from a summary-statistics file ask for.  With stat one of TWK_HIP_STAT_* and 1 <= k <= TWK_HIP_TOPK_MAX:
 *   the PARTNERS of variant v are the variants w for which twk_hip_ld_region with these arguments would report a record for {v, w}: both
 *                ends of a record count, as in the score, and the variant itself is no partner;
 *   the VALUE of a partner is that record's statistic - signed r (R with D's sign), r2, D or D' - computed in double and rounded once to
 *                float32: the bits twk_hip_ld_matrix writes at (v, w);
 *   the LIST of v is its partners ordered by |value| descending, compared as float32; of two partners with the same |value| the one
 *                with the smaller index in file order comes first (+x and -x tie); the list is cut at k.
 *   idx          HOST array of n_variants * k entries, overwritten: row v at v * k, the partners' indices as uploaded
 *   val          HOST array of n_variants * k floats, overwritten: their signed values
 * Slots that are not used - fewer than k partners, a variant outside the slice - hold TWK_HIP_NO_PARTNER and +0.0f, behind the used ones.
 * THE SELECTION IS EXACT AND HAS NO ORDER (ld_topk.hip.h, ld_topk_key.h): a candidate is one 64-bit integer key whose order is the
 * list's, selected with integer atomic maxima; the same bytes for any tile_variants, any launch order and any repeat, and no
 * floating-point atomic is used.  A shard (part / n_parts) returns the lists over its own pairs: the shards' lists merged under the
 * same order and cut at k are the lists of the whole.
 * filters.minP must be >= 1: Fisher's test is not run.  Always the matrix form of the contraction (TWK_HIP_OPT_R2_SCREEN is ignored, as
 * for a score).  *n_pairs (may be NULL): pairs evaluated.  The context is left as it was.
 * TWK_HIP_E_INVALID before any launch, with nothing written: minP < 1, a NULL array, k == 0 or k > TWK_HIP_TOPK_MAX, an unknown stat, and
 * the region call's own argument errors; TWK_HIP_E_STATE before upload.  Device memory: k * 8 bytes per variant for the length of the
 * call (531,500 variants at k = 16: 68 MB, where the dense matrix would need 1.13 TB); TWK_HIP_E_NOMEM with the size in
 * twk_hip_last_error when the device cannot give it.  twk_hip_timing: the kernels count as the math stage (stats_ms, stats_launches,
 * variant_pairs).  twk_hip_topk_last: the time from the last launch's end to the unpacked lists (the copy of the keys and their
 * unpacking on the host) and the lists' bytes on the device, of the context's last twk_hip_ld_topk call.  There is NO reference
 * counterpart. */
#define TWK_HIP_TOPK_MAX 32
#define TWK_HIP_NO_PARTNER 0xFFFFFFFFu
int twk_hip_ld_topk(twk_hip_ctx* ctx, int mode, const twk_hip_filters* filters,
                    uint32_t a0, uint32_t nA, uint32_t b0, uint32_t nB, int32_t triangle,
                    uint32_t part, uint32_t n_parts, uint32_t tile_variants,
                    int32_t window, uint32_t l_window,
                    int32_t stat, uint32_t k, uint32_t* idx /*[n_variants * k]*/, float* val /*[n_variants * k]*/, uint64_t* n_pairs);
int twk_hip_topk_last(const twk_hip_ctx* ctx, double* unpack_ms, uint64_t* list_bytes);

/* The sample relationship matrix: sample by sample instead of variant by variant - what a cohort user computes before any LD, to find
 * duplicates and relatives.  The same AND + popcount contraction with the reduced axis turned round: the genotype matrix is transposed
 * on the device into bit planes of the SAMPLES over the variants in use, the count kernel contracts them, and an epilogue turns the plane
 * products of a sample pair into exact integer counts and one statistic.
 *   variants, n_use   the variants in use, indices as uploaded, strictly ascending; NULL: all of them (n_use is ignored)
 *   sA0, nSA, sB0, nSB  the sample rows [sA0, sA0 + nSA) and columns [sB0, sB0 + nSB) of the matrix
 * For two samples a, b let g be a sample's ALT-allele count at a variant (0, 1, 2; phase is ignored); a sample is missing at a variant
 * when its mask bits are set.  Over the variants in use at which BOTH samples are non-missing:
 *   n       the number of such variants            ibs0    the number with {g_a, g_b} = {0, 2}
 *   ibs2    the number with g_a == g_b             hethet  the number with g_a == g_b == 1
 *   het_a   the number with g_a == 1               het_b   the number with g_b == 1          (ibs1 = n - ibs0 - ibs2)
 * The diagonal is a pair like any other: ibs2 = n, ibs0 = 0, hethet = het_a = het_b.  A statistic is ONE double division of integers
 * formed in 64 bits (the build has no fast-math: IEEE division, the bits numpy's division of the same integers gives):
 *   TWK_HIP_REL_IBS   (n + ibs2 - ibs0) / (2 n)                mean allele sharing: PLINK's 2 - |g_a - g_b|, averaged and halved
 *   TWK_HIP_REL_IBS0  ibs0 / n
 *   TWK_HIP_REL_KING  (hethet - 2 ibs0) / (het_a + het_b)      the KING-robust kinship as PLINK 2's --make-king forms it; signed numerator
 * and an entry whose denominator is 0 is `fill`, bit for bit.
 *   out     HOST array of nSA rows of ld >= nSB doubles, or NULL;  counts  HOST array of nSA rows of ld_counts >= nSB entries, or NULL
 *           (not both NULL).  Columns beyond nSB are not written.  A caller with more samples than one output fits asks for rectangles;
 *           several GPUs are the caller's rectangles on several contexts.
 *   *n_sample_pairs (may be NULL)  the pairs evaluated: nSA * nSB, or nSA (nSA + 1) / 2 when the call is a square on the diagonal
 *           (sA0 == sB0 and nSA == nSB) - then only the tiles on or above the diagonal are contracted and every pair fills (a, b) and
 *           (b, a), het_a and het_b swapped.
 * The planes are two a sample (het, hom-alt) when no variant in use has missing genotypes and three (het, hom-alt, non-missing) when one
 * has; they live for the length of the call (re-transposing reads the raw matrix once, little next to the contraction), and the sample
 * pair space is walked in super-tiles, so the count matrix stays bounded whatever the sample count.  Plain stores, every entry by
 * exactly one lane of one launch, no atomics: two calls return the same bytes.  The context is afterwards as it was: no option, no
 * variant plane set and no record-path state changes.
 * TWK_HIP_E_INVALID before any launch: both outputs NULL, ld or ld_counts below nSB, an empty sample slice or one beyond the last sample,
 * n_use == 0 with a list, a list that is not strictly ascending or reaches beyond the last variant, an unknown stat; TWK_HIP_E_STATE
 * before twk_hip_set_problem; TWK_HIP_E_NOMEM with the size in twk_hip_last_error when the planes, the count matrix or the output do
 * not fit the device.  twk_hip_timing: the count launches count as count_ms, count_launches and row_pairs, the epilogue as stats_ms and
 * stats_launches; the transposition is reported by twk_hip_relationship_last.
 * The reference's `relationship` (lib/relationship.h) is NOT reproduced: its inner loop skips the first sample of every run, it scores
 * het / het as 2 inside a run and 1 across runs, its mirroring leaves column 0 empty and it divides by the number of variants whatever
 * is missing.  The statistics here are defined from the integer counts above. */
enum { TWK_HIP_REL_IBS = 0, TWK_HIP_REL_IBS0 = 1, TWK_HIP_REL_KING = 2 };
typedef struct { uint32_t n, ibs0, ibs2, hethet, het_a, het_b; } twk_hip_rel_counts;
int twk_hip_relationship(twk_hip_ctx* ctx,
        const uint32_t* variants, uint32_t n_use,          /* variants in use, strictly ascending; NULL: all (n_use ignored) */
        uint32_t sA0, uint32_t nSA, uint32_t sB0, uint32_t nSB,  /* sample rows x sample columns */
        int32_t stat, double fill,
        double* out, uint64_t ld,                          /* nSA rows of ld >= nSB doubles; may be NULL */
        twk_hip_rel_counts* counts, uint64_t ld_counts,    /* likewise; may be NULL (not both) */
        uint64_t* n_sample_pairs);
/* Of the context's last twk_hip_relationship call: planes a sample (2 or 3), the device time of the transposition in ms and the bytes of
 * the plane set (any may be NULL). */
int twk_hip_relationship_last(const twk_hip_ctx* ctx, int32_t* planes_per_sample, double* transpose_ms, uint64_t* plane_bytes);

/* Multi-GPU runs: keep the survivors of twk_hip_ld_all / twk_hip_ld_region on the device.  With on != 0 the
 * record sink of those calls is not invoked; the survivors of every tile are appended (each tile in (idxA, idxB)
 * order, tiles in the order they finish) to one device buffer that twk_hip_device_records() returns, so that a
 * gather over RCCL can send them GPU to GPU and only the writer rank copies them to host memory, once.  This is
 * the per-worker output block of the reference (twk_ld_engine::blk_f / blk_r, lib/ld/ld_engine.h:321, flushed
 * into the shared writer at ld_engine.cpp:1270-1281) held in HBM until the gather.  Every call of
 * twk_hip_set_device_sink (on or off) empties the buffer.  *records is device memory owned by the ctx, valid
 * until the next compute call or twk_hip_set_device_sink; NULL when *n == 0. */
int twk_hip_set_device_sink(twk_hip_ctx* ctx, int on);
int twk_hip_device_records(twk_hip_ctx* ctx, const twk_hip_record** records, uint64_t* n);

/* One process, several GPUs (`tomahawk calc` with TWK_HIP_GPUS = n and engine option "gather" = 1): gather the device sinks of n
 * contexts - one per GPU, each with twk_hip_set_device_sink on and its region calls done - into the device sink of ctxs[dst], GPU to
 * GPU over RCCL: one communicator clique per set of devices (ncclCommInitAll, kept for the life of the process), then ONE group of
 * exact-size ncclSend / ncclRecv on the contexts' copy streams - no padding to a common size, no host hop.  Afterwards ctxs[dst]'s
 * sink holds its own records followed by those of the other contexts in the order of ctxs[]; the others' sinks are empty.
 * This is the north star's "final RCCL gather of .two output blocks over xGMI" inside the C++ product; it replaces every slave's
 * flush of its output block into the shared writer (lib/ld/ld_engine.cpp:1742-1802).  librccl is opened on first use (dlopen), never
 * linked: twk_hip_gather_backend() says what was found (and NCCL_DEBUG is set to NONE unless the caller has set it: RCCL otherwise
 * prints a banner to stdout when its first communicator comes up).  n == 1: nothing to move - unless flags has TWK_HIP_GATHER_SELF_LOOP, which
 * sends the one context's records from its sink to itself through the same group of calls (what a one-GPU box can exercise of the
 * path).  *transfer_ms (may be NULL): the transfers' duration on the destination's stream (HIP events).  Everything gathered must fit
 * the destination's HBM beside its problem (TWK_HIP_E_NOMEM otherwise: the caller falls back to per-GPU copies to the host). */
enum { TWK_HIP_GATHER_SELF_LOOP = 1 };
int twk_hip_gather_records(twk_hip_ctx* const* ctxs, uint32_t n, uint32_t dst, int32_t flags, uint64_t* n_records, double* transfer_ms);
const char* twk_hip_gather_backend(void);      /* "rccl <version code>" or "unavailable (<why>)" */
/* Hand what the device sink holds to `sink` on the host - in pieces of at most 2^20 records through the engine's pinned staging, in the
 * order they lie in the sink - and empty it.  (The records of a gathered run leave the destination GPU this way, once.) */
int twk_hip_drain_device_sink(twk_hip_ctx* ctx, twk_hip_record_sink sink, void* user, uint64_t* n_records);

/* The row band [row_begin,row_end) that shard `part` of `n_parts` owns in a region of
 * n_rows x n_cols variants (triangle != 0: col > row only, n_rows == n_cols) and the
 * number of pairs in it.  Pure host arithmetic (no device needed): lets a launcher
 * or a test derive the multi-GPU partition that twk_hip_ld_all/ld_region use. */
int twk_hip_shard_rows(uint32_t n_rows, uint32_t n_cols, int32_t triangle, uint32_t part, uint32_t n_parts,
                       uint32_t* row_begin, uint32_t* row_end, uint64_t* n_pairs);

/* The planner behind twk_hip_ld_region on caller-supplied arrays - pure host arithmetic, no device, no ctx (csrc/hip/ld_plan.h): the
 * shard's rows, the columns every row reaches (window: same contig, |dpos| <= l_window; r2 band: from the allele counts `popc`, positions
 * in order of minor allele count), and the launches (tile descriptors) that cover them; the first *n_band_launches of them are band
 * launches (fused form: rows x all the columns they reach).  meta / popc: one entry per position of the index space [0, n_variants).
 * tiles: room for `capacity` descriptors (TWK_HIP_E_OVERFLOW with *n_tiles = the number needed); lo / hi: nA entries each or NULL (filled
 * in window / band mode: row a0 + r reaches columns [b0 + lo[r], b0 + hi[r])).  Replaces twk_ld_balancer::Build and the block-pair
 * ticker (lib/ld/ld_balancing.h:23-80, 176-233) for one GPU's share; exported so that the partition can be tested and inspected
 * without a GPU (tests/test_plan.py). */
typedef struct {
	uint32_t n_samples;
	int32_t  planes_per_variant;  /* plane rows per variant of the mode's plane set: 1 phased, 2 unphased (masked: 2 / 3) */
	uint32_t k_chunks;            /* 128-byte chunks of a plane row (band launches are sized by tiles x chunks)            */
	uint32_t resident_blocks;     /* count-kernel blocks the chip holds at once (2 per CU: 512)                          */
	int32_t  screen;              /* 0 none, 1 r2 band for PhasedMath, 2 for UnphasedMath                                 */
	int32_t  fused;               /* the mode's launches run the fused count -> screen form                              */
	int32_t  phased_math;
	int32_t  band_launch, band_reverse;   /* the options of the same names */
	int32_t  _pad;
	int64_t  band_work_log2, band_max_launches;
	double   minR2;
} twk_hip_plan_env;
int twk_hip_plan_region(const twk_hip_plan_env* env, const twk_hip_variant_meta* meta, const uint32_t* popc, uint32_t n_variants,
                        uint32_t a0, uint32_t nA, uint32_t b0, uint32_t nB, int32_t triangle, uint32_t part, uint32_t n_parts,
                        uint32_t tile_variants, int32_t window, uint32_t l_window,
                        twk_hip_tile_desc* tiles, uint32_t capacity, uint32_t* n_tiles, uint32_t* n_band_launches,
                        uint32_t* row_begin, uint32_t* row_end, uint64_t* n_pairs, uint32_t* lo, uint32_t* hi);
/* The same for the two-product walk of an unscreened UnphasedMath call (screen = 0, planes_per_variant = 2, a triangle): het /
 * hom = het and hom-alt carriers per position of the index space, which is in order of minor allele count; two_margin: what the square
 * root of the screen's bound is shrunk to when the planner asks which rows can take two products (0: the engine's 0.95).  *two_end
 * (may be NULL): the row, a multiple of 128, the triangle is cut at - no launch straddles it, launches in front of it may take two
 * products.  het == hom == NULL: twk_hip_plan_region. */
int twk_hip_plan_region_two(const twk_hip_plan_env* env, const twk_hip_variant_meta* meta, const uint32_t* popc, const uint32_t* het, const uint32_t* hom, double two_margin,
                            uint32_t n_variants, uint32_t a0, uint32_t nA, uint32_t b0, uint32_t nB, int32_t triangle, uint32_t part, uint32_t n_parts,
                            uint32_t tile_variants, int32_t window, uint32_t l_window,
                            twk_hip_tile_desc* tiles, uint32_t capacity, uint32_t* n_tiles, uint32_t* n_band_launches,
                            uint32_t* row_begin, uint32_t* row_end, uint64_t* n_pairs, uint32_t* lo, uint32_t* hi, uint32_t* two_end);
/* ... with the row operand of the walk's two-product launches named: carrier == 0: the row variants' H planes (twk_hip_plan_region_two); != 0: their
 * carrier planes H | Q, as the engine's launches take them on rows of more than 128 K chunks (option "carrier") - the cut is then asked of the carrier
 * screen (csrc/hip/ld_two_screen.h: screen2c_expected_keeps) and lies further on. */
int twk_hip_plan_region_two_operand(const twk_hip_plan_env* env, const twk_hip_variant_meta* meta, const uint32_t* popc, const uint32_t* het, const uint32_t* hom, double two_margin,
                                    int32_t carrier, uint32_t n_variants, uint32_t a0, uint32_t nA, uint32_t b0, uint32_t nB, int32_t triangle, uint32_t part, uint32_t n_parts,
                                    uint32_t tile_variants, int32_t window, uint32_t l_window,
                                    twk_hip_tile_desc* tiles, uint32_t capacity, uint32_t* n_tiles, uint32_t* n_band_launches,
                                    uint32_t* row_begin, uint32_t* row_end, uint64_t* n_pairs, uint32_t* lo, uint32_t* hi, uint32_t* two_end);
/* ... and with the one-product launches of the carrier form (option "one"): one != 0 (read only with carrier != 0): the rows in front of the cut are
 * walked in blocks of one_rows variants (a multiple of 128; 0: the engine's default), and a block's columns from the diagonal to its one_end - where
 * the screen's lower test at S >= 0 stops passing for the block's last row (csrc/hip/ld_two_screen.h: screen1c_lower_ok), rounded down to 128
 * variants - are launches with twk_hip_tile_desc::one set. */
int twk_hip_plan_region_two_form(const twk_hip_plan_env* env, const twk_hip_variant_meta* meta, const uint32_t* popc, const uint32_t* het, const uint32_t* hom, double two_margin,
                                 int32_t carrier, int32_t one, uint32_t one_rows, uint32_t n_variants, uint32_t a0, uint32_t nA, uint32_t b0, uint32_t nB, int32_t triangle, uint32_t part, uint32_t n_parts,
                                 uint32_t tile_variants, int32_t window, uint32_t l_window,
                                 twk_hip_tile_desc* tiles, uint32_t capacity, uint32_t* n_tiles, uint32_t* n_band_launches,
                                 uint32_t* row_begin, uint32_t* row_end, uint64_t* n_pairs, uint32_t* lo, uint32_t* hi, uint32_t* two_end);

/* ... and with the fine walk (option "walk_fine"; read only with carrier != 0): fine != 0: the cut is asked of the carrier screen that holds QQ to
 * min(qA, qB, CQ), a block in front of the cut has its one_end per tile row of 128 variants - a staircase: its one-product launches list the tiles in
 * front of it, its two-product launches the tiles behind it - and the blocks of the rows [*two_end, *two_last) take a two-product launch from the
 * diagonal to their rows' two_reach and three products behind it.  notes (may be NULL; `capacity` entries): per launch, bits 0-1: 0 the whole
 * rectangle, 1 the columns in front of its rows' staircase border, 2 those from it on; bit 2: a two-product launch behind the cut.  stair (may be
 * NULL; nA entries): the border of row a0 + r, relative to b0 (0: none).  fine == 0: twk_hip_plan_region_two_form. */
int twk_hip_plan_region_walk(const twk_hip_plan_env* env, const twk_hip_variant_meta* meta, const uint32_t* popc, const uint32_t* het, const uint32_t* hom, double two_margin,
                             int32_t carrier, int32_t one, uint32_t one_rows, int32_t fine, uint32_t n_variants, uint32_t a0, uint32_t nA, uint32_t b0, uint32_t nB, int32_t triangle, uint32_t part, uint32_t n_parts,
                             uint32_t tile_variants, int32_t window, uint32_t l_window,
                             twk_hip_tile_desc* tiles, uint32_t capacity, uint32_t* n_tiles, uint32_t* n_band_launches,
                             uint32_t* row_begin, uint32_t* row_end, uint64_t* n_pairs, uint32_t* lo, uint32_t* hi, uint32_t* two_end,
                             uint32_t* two_last, uint8_t* notes, uint32_t* stair);

/* Fisher's exact test on n caller-supplied 2x2 tables (tables[4*i + {0,1,2,3}] = n11, n12, n21, n22), two-sided P
 * into p_two_sided[i]: kt_fisher_exact (lib/fisher_math.cpp:231-267) as the pair math calls it
 * (ld_engine.cpp:1222-1226, :1656-1658), through the engine's own Fisher kernels: the reference's walk, one table per
 * lane, behind the search for its starting points.  in_given_order == 0: as the pair math runs it, the walks in the order
 * of their length; != 0: in the order of `tables` (same P, bit for bit: a measurement switch).  Needs
 * twk_hip_set_problem first (the log-factorial table covers counts up to 2 * n_samples + 15; larger counts take
 * lgamma itself).  *kernel_ms (may be NULL): the kernels' duration (HIP events).  A parity and measurement entry
 * point: the pair math reaches the same kernels internally. */
int twk_hip_fisher_exact(twk_hip_ctx* ctx, const int32_t* tables, uint64_t n, double* p_two_sided,
                         int32_t in_given_order, float* kernel_ms);

/* ---- switches ---------------------------------------------------------- */
/* Measurement and test switches of one ctx, by name.  The library reads NO environment variable: a process that
 * embeds it gets the documented defaults unless it calls this.  There is no reference counterpart (the reference's
 * closest relative is the compile-time SLAVE_DEBUG_MODE / SIMD_AVAILABLE switches, lib/ld/ld_engine.h:20-24).
 * The keys, their defaults, ranges and meaning are ONE table in the engine (TWK_HIP_OPTIONS, csrc/hip/twk_hip.hip), readable through
 * twk_hip_option_describe() below and printed as the table of INTEGRATION.md 1 (tests/test_docs_consistency.py keeps the document in
 * step with it).  In short: "fused", "three", "uz", "two", "carrier", "one", "prefix" pick the form of the contraction
 * ("prefix_margin" and "prefix_sigma" are the two questions the prefix contraction's planner asks for a tile's stop on its 128-point grid,
 * "prefix_stop" plus "prefix_substop" a test hook that puts every tile's stop on one point of it: DESIGN 3.1c); "lists", "list_max", "probe", "probe_zone",
 * "probe_lds" the carrier-list passes for rare variants; "band_*" the launches of fused runs; "patch_rows" / "patch_cols" / "seg" /
 * "xcd_queues" / "skip_pad" / "count_min_chunks" / "cand_chunk" the count kernel's work order; "fisher_*" Fisher's test;
 * "async_delivery", "deliver_buffers" the engine's delivery thread; "record_cap", "deliver_fail_*_at" are test hooks; "timeline" a log.
 * Keys of the host side (`tomahawk calc --engine-option`, twk_ld::SetEngineOption - handled in csrc/host/twk_ld.cpp, unknown to this
 * function): "force_device", "progress_ms", "map_output", "emit_workers", "emit_backlog_mb", "emit_queue_pieces", "record_codec", "direct_output" (INTEGRATION.md 1).
 * None of them changes a record (tests/test_gpu_fused.py, test_gpu_lists.py); "lists" / "list_max" drop the derived
 * plane sets, which are rebuilt on next use.  Unknown key or value out of range: TWK_HIP_E_INVALID. */
int twk_hip_set_option(twk_hip_ctx* ctx, const char* key, int64_t value);
int twk_hip_get_option(const twk_hip_ctx* ctx, const char* key, int64_t* value);
/* Entry `index` (0, 1, ... until TWK_HIP_E_INVALID) of the engine's option table: key, default, range, one line of meaning (static strings;
 * any pointer may be NULL).  Needs no device and no ctx. */
int twk_hip_option_describe(uint32_t index, const char** key, int64_t* dflt, int64_t* lo, int64_t* hi, const char** meaning);

/* ---- measurement ------------------------------------------------------ */
/* Cumulative device time (HIP events on the engine's own stream) and launch
 * count of the dominant kernel (count-tile) and of the math kernel since the
 * last reset, plus the algorithmic units they processed. */
typedef struct {
	double   count_ms;      /* sum of count-kernel durations                     */
	double   stats_ms;      /* sum of math/filter-kernel durations (a band launch: up to and including the sort of its survivors) */
	uint64_t count_launches;
	uint64_t stats_launches;
	uint64_t row_pairs;     /* plane-row pairs contracted by the count kernel    */
	uint64_t variant_pairs; /* variant pairs evaluated by the math kernel        */
	uint64_t words_per_row; /* 32-bit words contracted per row pair (unpadded)   */
	uint64_t fused_launches;/* count launches that ran the fused count -> r2 screen form (short rows,
	                           phased math: no count matrix, candidates only)    */
	uint64_t candidates;    /* list slots those launches handed to the math kernel:
	                           the pairs that passed the screen, plus the slots a wave
	                           had reserved and not used when its launch ended      */
	double   list_ms;       /* sum of carrier-list intersection kernel durations (rare variants at very large sample
	                           counts: the device's twk_igt_list / PhasedListVector, core.h:517-672, ld_engine.cpp:185-267) */
	uint64_t list_launches;
	uint64_t list_pairs;    /* variant pairs decided by list intersection instead of the dense contraction */
	double   probe_ms;      /* sum of the probe kernel's durations: a rare variant's carrier list against the bitvector rows of variants
	                           that keep no list (K1's asymmetric path, ld_engine.cpp:230-242) */
	uint64_t probe_launches;
	uint64_t probe_pairs;   /* variant pairs decided that way */
	uint64_t count_shader_cycles; /* what the count kernel's blocks lived for, summed over the blocks: shader clock cycles ...   */
	uint64_t count_wall_ticks;    /* ... and ticks of the constant 100 MHz counter.  cycles / ticks x 100 MHz = the clock the
	                                 launches really ran at (a chip that was idle needs ~20 ms of load to reach its 2.4 GHz) */
	uint64_t three_launches;      /* count launches that ran the three-product form of the plain unphased planes: per word and
	                                 variant pair HH = popc(H_A & H_B) and S = popc(Q_A & C_B) + popc(C_A & Q_B), C = H | Q - what
	                                 UnphasedMath's r2 screen reads (ld_engine.cpp:1363-1375 via minhap / maxhap) - instead of the four
	                                 products HH, HQ, QH, QQ; the reference's list kernel likewise takes one popcount and the other
	                                 cells from the margins (ld_engine.cpp:244-246) */
	uint64_t three_row_pairs;     /* ... and the plane-row pairs of those launches (of row_pairs): they executed 3/4 of the
	                                 AND+popcounts row_pairs x words_per_row stands for (one v_and / v_bitop3 + one v_bcnt each) */
	uint64_t recount_candidates;  /* pairs that passed the three-product screen and had their four products counted afresh */
	uint64_t outlier_launches;    /* count launches the outlier watch flagged (twk_hip_launch_log)                          */
	double   finish_ms;           /* (ABI 5) the calling thread's wall time between a launch's last kernel and the hand-over of its
	                                 records: device sort, copy to the host, the sink (launches the delivery thread takes: up to
	                                 their copy aside on the device) - summed over the launches                              */
	uint64_t two_launches;        /* Appended behind the ABI 5 layout, and TWK_HIP_ABI_VERSION stays 5: twk_hip_timing_get writes sizeof(twk_hip_timing) of THIS
	                                 header, so a caller compiled against an older one must be rebuilt - the version check does not catch it
	                                 (nothing but this library's own binding and host code, built with it, reads the struct).
	                                 Count launches that ran the two-product form: HH and HQ of the row variants' H planes
	                                 against the column variants' H and Q rows.  Their row_pairs are the plane-row pairs they really
	                                 contracted - one row x two rows per variant pair - and they are no part of three_launches /
	                                 three_row_pairs                                                                          */
	uint64_t prefix_launches;     /* (appended likewise) Two- and three-product launches that contracted their tiles over a prefix of the rows
	                                  and whose candidate list held - one that flooded and was redone over whole rows is not counted.  They stay part of two_launches / three_launches, and their row_pairs / three_row_pairs
	                                 count full-row equivalents: plane-row pairs x chunks contracted / chunks per row, summed over the
	                                 tiles and rounded down once per launch - so that row_pairs x words_per_row stays the work executed */
	uint64_t prefix_chunks;       /* K chunks those launches' tiles were contracted over ...                                   */
	uint64_t prefix_chunks_full;  /* ... and what whole rows would have been                                                   */
	uint64_t carrier_launches;    /* (appended likewise) Two-product launches whose row operand was the row variants' carrier plane H | Q
	                                 in the H plane's place (CH and CQ for HH and HQ).  They stay part of two_launches, with
	                                 the same row_pairs accounting: one row x two rows per variant pair                        */
	uint64_t one_launches;        /* (appended likewise) Carrier launches that contracted one product a pair - the carrier rows of both variants,
	                                 CC = CH + CQ - in front of their rows' one_end.  They stay part of two_launches and
	                                 carrier_launches; their row_pairs are their variant pairs, one row x one row, in full-row equivalents
	                                 under stops                                                                              */
	uint64_t uz_launches;         /* (appended likewise) Three-product launches through a matrix that contracted U = popc(H_A | H_B) and
	                                 Z = popc((Q_A ^ Q_B) & ~(H_A | H_B)) in the place of HH and S (option "uz"): two popcounts a
	                                 word of a variant pair where the products are three.  They stay part of three_launches ...           */
	uint64_t uz_row_pairs;        /* ... and their plane-row pairs part of three_row_pairs and row_pairs, counted as theirs; a word of them
	                                 issued v_or + v_bcnt + v_bitop3 + v_bcnt, 12 SIMD cycles a variant pair where three products are 18   */
	uint64_t uz_split_units;      /* ... and their units of work beyond one a tile: the parts of tiles cut along K at the end of a launch,
	                                 whose U and Z are added into the matrix with atomics (0: every tile was contracted by one block)      */
} twk_hip_timing;
/* Progress of twk_hip_ld_all / twk_hip_ld_region: `cb` runs on the calling thread after every tile
 * with the variant pairs finished so far in the current call and the tile counts.  Replaces the
 * counters the reference's ticker thread polls every 30 s (lib/ld/ld_progress.h:40-86: n_var, n_out).
 * cb == NULL switches it off. */
typedef void (*twk_hip_progress_cb)(void* user, uint64_t pairs_done, uint32_t tiles_done, uint32_t tiles_total);
int twk_hip_set_progress(twk_hip_ctx* ctx, twk_hip_progress_cb cb, void* user);

/* The count launches one by one, since the last twk_hip_timing_reset (a ring of the last 4096): what the engine's outlier watch
 * looks at.  A launch is an outlier when its time per unit of work (row_pairs x words_per_row, the three-product form's at 3/4)
 * exceeds 1.4 x the median of the launches of its own kind and row length before it (at least 8 of them, launches of >= 0.3 ms);
 * option "timeline" >= 1 prints such a launch - with the shader clock its blocks ran at and how far apart the XCDs finished - on
 * stderr as it is found.  Measurement integrity (round 4 saw the same run take 1.7 x as long now and then); no reference counterpart. */
typedef struct {
	double   ms;                  /* HIP events around the count kernel                                        */
	double   shader_mhz;          /* clock the blocks ran at (0: not measured)                                 */
	double   xcd_finish_spread_us;/* last block of the last XCD to finish minus last block of the first one    */
	uint64_t row_pairs;           /* plane-row pairs contracted                                                */
	uint64_t candidates;          /* fused / three-product launches: pairs that passed the screen              */
	uint32_t words_per_row;
	uint32_t kind;                /* 0 four products -> matrix, 1 three products -> matrix, 2 fused PhasedMath,
	                                 3 fused UnphasedMath four products, 4 fused UnphasedMath three products,
	                                 5 two products -> matrix (row variants' H planes x column variants' H, Q) */
	uint32_t outlier;             /* != 0: flagged by the watch                                                */
	uint32_t uz;                  /* (in the place of padding) != 0: a kind-1 launch in the (U, Z) form (option "uz")          */
	/* Appended behind the ABI 5 layout with TWK_HIP_ABI_VERSION still 5 (existing callers' checks pin it): the entry grew, so the stride of the
	 * array twk_hip_launch_log fills changed - a caller compiled against the older header would misread every entry after the first and must be
	 * rebuilt; the version check does not catch it (only this library's own binding, built with it, reads the log). */
	uint64_t prefix_chunks;       /* a prefix launch: K chunks its tiles were contracted over ... (else 0)      */
	uint64_t prefix_chunks_full;  /* ... and what whole rows would have been; row_pairs is scaled by their ratio            */
	uint32_t carrier;             /* (appended likewise) != 0: a kind-5 launch whose row operand was the carrier plane H | Q   */
	uint32_t one;                 /* (in the place of padding) != 0: such a launch that contracted one product a pair, carrier rows on both axes */
} twk_hip_launch_stat;
/* Copies the most recent min(capacity, launches kept) entries, oldest first; *n_total: launches seen since the reset. */
int twk_hip_launch_log(twk_hip_ctx* ctx, twk_hip_launch_stat* out, uint32_t capacity, uint32_t* n_copied, uint64_t* n_total);

int twk_hip_timing_reset(twk_hip_ctx* ctx);
int twk_hip_timing_get(twk_hip_ctx* ctx, twk_hip_timing* out);

#ifdef __cplusplus
}
#endif
#endif /* TWK_HIP_H_ */
