# Build everything in-tree for gfx950 (MI355X).  hipcc cross-compiles without a GPU.
#   lib/libtwk_hip.so       HIP kernels + C ABI (include/twk_hip.h)
#   lib/libtomahawk_amd.so  host C++: .twk/.two formats, tomahawk::twk_ld, test C API
#   bin/tomahawk            `tomahawk calc` CLI
#   oracle/liboracle.so     CPU oracle (tests only)   oracle/_ref/  compiled reference (tests/baseline only)
HIPCC    ?= /opt/rocm/bin/hipcc
CXX      ?= g++
ARCH     ?= gfx950
PKG      := tomahawk_amd
LIBDIR   := $(PKG)/lib
BINDIR   := $(PKG)/bin
ZSTD_LIB ?= /usr/lib/x86_64-linux-gnu/libzstd.so.1
ZLIB     ?= /usr/lib/x86_64-linux-gnu/libz.so.1

HIP_SRC  := $(PKG)/csrc/hip/twk_hip.hip
HIP_DEPS := $(wildcard $(PKG)/csrc/hip/*.h) include/twk_hip.h
# -ffp-contract=off: the pair statistics must round like the reference's SSE4.2 build (ld_math.hip.h)
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-function

HOST_SRC := $(wildcard $(PKG)/csrc/host/*.cpp)
HOST_LIB_SRC := $(filter-out %/calc_main.cpp,$(HOST_SRC))
HOST_DEPS := $(wildcard $(PKG)/csrc/host/*.h) include/twk_hip.h
CXXFLAGS := -O2 -std=c++17 -fPIC -Wall -pthread -Iinclude -I$(PKG)/csrc/host

.PHONY: all hip host cli oracle tools clean asan asan-test tsan buffers-check matrix-check decay-check aggregate-check relate-check count-check two-check prefix-check annot-check form-check uz-check bandmat-check topk-check subset-check varsel-check blocks-check split-check
all: hip host cli oracle

hip: $(LIBDIR)/libtwk_hip.so
$(LIBDIR)/libtwk_hip.so: $(HIP_SRC) $(HIP_DEPS)
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -shared $(HIP_SRC) -o $@

host: $(LIBDIR)/libtomahawk_amd.so
$(LIBDIR)/libtomahawk_amd.so: $(HOST_LIB_SRC) $(HOST_DEPS) $(LIBDIR)/libtwk_hip.so
	@mkdir -p $(LIBDIR)
	$(CXX) $(CXXFLAGS) -shared $(HOST_LIB_SRC) -o $@ -L$(LIBDIR) -ltwk_hip $(ZSTD_LIB) $(ZLIB) -Wl,-rpath,'$$ORIGIN'
	ln -sf libtomahawk_amd.so $(LIBDIR)/libtomahawk.so      # the reference library's name (makefile:162-182), for -ltomahawk

cli: $(BINDIR)/tomahawk
$(BINDIR)/tomahawk: $(PKG)/csrc/host/calc_main.cpp $(LIBDIR)/libtomahawk_amd.so
	@mkdir -p $(BINDIR)
	$(CXX) $(CXXFLAGS) $< -o $@ -L$(LIBDIR) -ltomahawk_amd -ltwk_hip $(ZSTD_LIB) -Wl,-rpath,'$$ORIGIN/../lib'

oracle:
	$(MAKE) -C oracle all

tools: build/count_microbench build/valu_rate build/hbm_read_bw build/issue_test2 build/fisher_probe build/bank_test2 build/list_vs_dense build/probe_vs_dense build/shift64_probe build/issue_test3 build/lds_dma3_probe build/bitop3_probe build/sgpr_probe build/uz_probe
build/%: $(PKG)/csrc/tools/%.hip $(HIP_DEPS)
	@mkdir -p build
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 -ffp-contract=off -Ibuild $< -o $@
# (the probe's instruction streams with every register fixed by hand are written by a script)
build/bitop3_probe: build/bitop3_probe_gen.h
build/bitop3_probe_gen.h: $(PKG)/csrc/tools/bitop3_probe_gen.py
	@mkdir -p build
	python3 $< > $@
build/uz_probe: build/uz_probe_gen.h
build/uz_probe_gen.h: $(PKG)/csrc/tools/uz_probe_gen.py
	@mkdir -p build
	python3 $< > $@
build/sgpr_probe: build/sgpr_probe_gen.h
build/sgpr_probe_gen.h: $(PKG)/csrc/tools/sgpr_probe_gen.py
	@mkdir -p build
	python3 $< > $@

# AddressSanitizer + UBSan build of the host side (the GPU side cannot be sanitised on this pool): same sources,
# separate output directory; `make asan-test` runs the CPU test suite against it (python is not instrumented, so
# libasan is preloaded; leak checking is off because the interpreter and the HIP runtime never free their arenas).
ASAN_DIR := $(PKG)/lib_asan
SANFLAGS := -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined
asan: $(LIBDIR)/libtwk_hip.so
	@mkdir -p $(ASAN_DIR)
	$(CXX) $(CXXFLAGS) $(SANFLAGS) -shared $(HOST_LIB_SRC) -o $(ASAN_DIR)/libtomahawk_amd.so -L$(LIBDIR) -ltwk_hip $(ZSTD_LIB) $(ZLIB) -Wl,-rpath,'$$ORIGIN/../lib'
	$(CXX) $(CXXFLAGS) $(SANFLAGS) $(PKG)/csrc/host/calc_main.cpp -o $(ASAN_DIR)/tomahawk -L$(ASAN_DIR) -ltomahawk_amd -L$(LIBDIR) -ltwk_hip $(ZSTD_LIB) -Wl,-rpath,'$$ORIGIN:$$ORIGIN/../lib'
asan-test: asan
	LD_PRELOAD=$$($(CXX) -print-file-name=libasan.so):$$($(CXX) -print-file-name=libubsan.so) ASAN_OPTIONS=detect_leaks=0:abort_on_error=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 \
	TWK_HOST_LIB=$(abspath $(ASAN_DIR))/libtomahawk_amd.so TWK_CLI=$(abspath $(ASAN_DIR))/tomahawk python -m pytest tests -x -q -m "not gpu"

# ThreadSanitizer runs: the record emitter (worker pool, ordered placing step, backlog, mapped output) - the format and emitter sources with
# -fsanitize=thread around csrc/tools/emitter_tsan.cpp - and the engine's delivery queue (csrc/hip/twk_delivery.h) with the device operations
# stubbed (csrc/tools/delivery_tsan.cpp)
tsan:
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -pthread -fsanitize=thread -Iinclude -I$(PKG)/csrc/host $(PKG)/csrc/tools/emitter_tsan.cpp $(PKG)/csrc/host/twk_format.cpp \
		-o build/emitter_tsan $(ZSTD_LIB) $(ZLIB)
	TSAN_OPTIONS=halt_on_error=1 ./build/emitter_tsan
	$(CXX) -O1 -g -std=c++17 -pthread -fsanitize=thread $(PKG)/csrc/tools/delivery_tsan.cpp -o build/delivery_tsan
	TSAN_OPTIONS=halt_on_error=1 ./build/delivery_tsan

# The engine's buffer owners (csrc/hip/twk_buffers.h) with the allocator stubbed (csrc/tools/buffers_check.cpp): what is freed, when, and once
buffers-check:
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -Wall $(PKG)/csrc/tools/buffers_check.cpp -o build/buffers_check
	./build/buffers_check

# The LD matrix fill's slot arithmetic and guards (csrc/hip/ld_matrix_index.h) played lane by lane on the host (csrc/tools/matrix_index_check.cpp)
matrix-check:
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -Wall $(PKG)/csrc/tools/matrix_index_check.cpp -o build/matrix_index_check
	./build/matrix_index_check

# LD decay's bin index (csrc/hip/ld_decay_bin.h) against a naive restatement (csrc/tools/decay_bin_check.cpp), and the exact sums'
# quantisation, split and host conversion (csrc/hip/ld_exact_sum.h) for both split widths in use (csrc/tools/exact_sum_check.h)
decay-check:
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -Wall $(PKG)/csrc/tools/decay_bin_check.cpp -o build/decay_bin_check
	./build/decay_bin_check

# LD aggregate's packing (csrc/hip/ld_aggregate_bin.h) and ldaggregate's landscape (csrc/host/twk_aggregate_landscape.h) against a naive
# restatement (csrc/tools/aggregate_bin_check.cpp), and the same checks of the exact sums as decay-check (csrc/tools/exact_sum_check.h)
aggregate-check:
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -Wall $(PKG)/csrc/tools/aggregate_bin_check.cpp -o build/aggregate_bin_check
	./build/aggregate_bin_check

# The sample relationship's layout, transposition, count formulas and epilogue lanes (csrc/hip/ld_relate_index.h) against a naive
# restatement (csrc/tools/relate_index_check.cpp): host code only, under AddressSanitizer and UBSan
relate-check:
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined $(PKG)/csrc/tools/relate_index_check.cpp -o build/relate_index_check
	./build/relate_index_check

# The count launches' work table - tiles in patch order, units, queues, the packed layout - and the last-chunk rule (csrc/hip/ld_count_table.h)
# against a naive restatement and against the recorded order of tests/golden/count_tables.json (csrc/tools/count_table_check.cpp): host code
# only, under AddressSanitizer and UBSan
count-check:
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined $(PKG)/csrc/tools/count_table_check.cpp -o build/count_table_check
	./build/count_table_check tests/golden/count_tables.json

# The two-product form's host side (csrc/tools/two_check.cpp): its screens (csrc/hip/ld_two_screen.h: the H plane or the carrier plane H | Q as the
# row operand, or one product of the two variants' carrier planes) over every small genotype table, plan_one_end on random sorted margins, and the
# work table of a launch with one plane row per row variant and two per column variant against a naive restatement and the recorded order of
# tests/golden/count_tables_two.json; the fine walk's carrier screen (QQ <= min(qA, qB, CQ)) between three products and the carrier screen:
# host code only, under AddressSanitizer and UBSan
two-check:
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined $(PKG)/csrc/tools/two_check.cpp -o build/two_check
	./build/two_check tests/golden/count_tables_two.json

# The prefix contraction's host side (csrc/tools/prefix_check.cpp): its screens (csrc/hip/ld_two_screen.h) over every pair of a small prefix and a
# small suffix genotype table, the work table with per-tile stops (csrc/hip/ld_count_table.h) against a naive restatement and against the table
# built without stops, and the planner's stops (csrc/hip/ld_plan.h) on the headline's frequency law - once with the H plane and once with the
# carrier plane as the two-product launches' row operand; the grid of 128 stops against a naive restatement for rows of 1 .. 2,000 chunks, the
# screens at every fine stop, and the planner at four settings of grid and margin; the fine walk (option "walk_fine"): its carrier prefix screen
# between three products and the carrier screen, the planner's report with and without it, and its plans on random margins - every pair in exactly
# one launch and on its side of the staircase: host code only, under AddressSanitizer and UBSan
prefix-check:
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined $(PKG)/csrc/tools/prefix_check.cpp -o build/prefix_check
	./build/prefix_check

# The partitioned LD score's term, its split width and the block's index arithmetic (csrc/hip/ld_annot_term.h) against llrint, the exact
# sums' checks (csrc/tools/exact_sum_check.h) and a whole block played on the host (csrc/tools/annot_term_check.cpp): host code only,
# under AddressSanitizer and UBSan
annot-check:
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined $(PKG)/csrc/tools/annot_term_check.cpp -o build/annot_term_check
	./build/annot_term_check

# Who may take which form of a count launch (csrc/hip/ld_form.h): decide_form over every combination of facts and grants, the transitions of
# CallForms::gave_up, the ladder a redone tile descends, the choice of the two-product launches' row operand, the thresholds and the sample ladder
# (decide_wants) under scripted samplers, and the (U, Z) attribute of a three-product launch through a matrix (option "uz")
# (csrc/tools/form_check.cpp): host code only, under AddressSanitizer and UBSan
form-check:
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined $(PKG)/csrc/tools/form_check.cpp -o build/form_check
	./build/form_check

# The (U, Z) form of the three-product contraction (csrc/hip/ld_count_uz.hip.h) on the host: the conversion its screen runs (csrc/hip/ld_two_screen.h:
# uz_to_hh_s, uz_prefix_to_hh_s) against the products - every 3 x 3 table of up to 7 samples, every prefix and suffix table of up to 4 + 4 samples with
# screen3_keeps / screen3_prefix_keeps on both, and zero-padded bit-plane rows word by word over every prefix (csrc/tools/uz_check.cpp): host code only,
# under AddressSanitizer and UBSan
uz-check:
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined $(PKG)/csrc/tools/uz_check.cpp -o build/uz_check
	./build/uz_check

# The banded LD matrix's layout against its O(n^2) definition, and the fill's slot arithmetic, guards and dead-block test
# (csrc/hip/ld_bandmat_index.h) played lane by lane against an array of write counts with a border (csrc/tools/bandmat_index_check.cpp):
# host code only, under AddressSanitizer and UBSan
bandmat-check:
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined $(PKG)/csrc/tools/bandmat_index_check.cpp -o build/bandmat_index_check
	./build/bandmat_index_check

# The top-k partners' key against the comparator of its definition, the cascade played step by step under random interleavings with stale
# threshold reads, and the kernel's two levels (csrc/hip/ld_topk_key.h) against a sort (csrc/tools/topk_key_check.cpp): host code only,
# under AddressSanitizer and UBSan
topk-check:
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined $(PKG)/csrc/tools/topk_key_check.cpp -o build/topk_key_check
	./build/topk_key_check

# The sample selection's table, compress and split by output words (csrc/hip/ld_subset_index.h) played block by block and lane by lane
# against a field-by-field gather and an array of write counts with a border (csrc/tools/subset_index_check.cpp): host code only, under
# AddressSanitizer and UBSan
subset-check:
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined $(PKG)/csrc/tools/subset_index_check.cpp -o build/subset_index_check
	./build/subset_index_check

# The variant selection's predicate, word counts and gather walk (csrc/hip/ld_varsel_index.h): the predicate with its equality boundaries
# against a restatement, every block and lane of the row gather against a row-by-row copy and an array of write counts with a border
# (csrc/tools/varsel_index_check.cpp): host code only, under AddressSanitizer and UBSan
varsel-check:
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined $(PKG)/csrc/tools/varsel_index_check.cpp -o build/varsel_index_check
	./build/varsel_index_check

# Haplotype blocks' host side (csrc/hip/ld_block_ci.h): the D' bounds' scan against a long double restatement (dmax == 0, a zero cell, D == 0,
# A and B swapped, fractional counts), the byte stores of the bounds' kernel lane by lane against arrays of write counts with a border, the
# prefix counts, the candidates' running sums and small-m rules against the contract with every pair counted, the sort key's order, and the
# walk played with lanes running ahead (csrc/tools/blocks_check.cpp): host code only, under AddressSanitizer and UBSan
blocks-check:
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -Wall -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined $(PKG)/csrc/tools/blocks_check.cpp -o build/blocks_check
	./build/blocks_check

# LD splitting's host side (csrc/hip/ld_split_index.h): every lane of the prefix, block-sum, layer and backtrack kernels - the wave scan and
# its carry, the saturation rule, the layers' ranges, the LDS windows and their bounds, the smallest-d rule - against a direct evaluation of
# the definition with arrays that count their writes, and tiny cases against an enumeration of all partitions (csrc/tools/split_check.cpp):
# host code only, under AddressSanitizer and UBSan
split-check:
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -Wall -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined $(PKG)/csrc/tools/split_check.cpp -o build/split_check
	./build/split_check

clean:
	rm -rf $(LIBDIR) $(BINDIR) $(ASAN_DIR) build
	$(MAKE) -C oracle clean
