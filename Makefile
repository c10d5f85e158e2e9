# Top-level build: the MI355X scorer library (HIP kernels + C-ABI + C++ host-side scorer
# classes), the C++ protocol test driver, and the (test-only) oracle.  No cmake; hipcc for gfx950.
ROCM_PATH ?= /opt/rocm
HIPCC    ?= $(ROCM_PATH)/bin/hipcc
ARCH     ?= gfx950
BUILD     = build
LIBDIR    = rasr_amd/lib
HIPFLAGS  = --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-result
# quantized kernels: MFMA results straight into VGPRs (gfx950 has one unified register file),
# so the v_lshl_add / v_min3 epilogue reads them without v_accvgpr_read copies.
I8FLAGS   = -mllvm -amdgpu-mfma-vgpr-form
# float kernels: default AGPR accumulators (measured faster for the f32 MFMA chains), see DESIGN.md "Measurements"
F32FLAGS  =
# split-f16 float kernel; no SLP packing: the diagonal-sum epilogue's adds were packed into v_pk_add_f32 /
# v_pk_mul_f32, which issue slower than two scalar ops beside the MFMAs (A/B: -1.0 %; no packed ops elsewhere)
SPLITFLAGS = -mllvm -amdgpu-mfma-vgpr-form -fno-slp-vectorize
HOSTFLAGS = -O2 -std=c++17 -fPIC -ffp-contract=off -Wall

SRC       = rasr_amd/csrc
HDRS      = include/rasr_gmm.h $(SRC)/gmm_presel.hh $(SRC)/gmm_prepare.hh $(SRC)/gmm_kernels.hh $(SRC)/gmm_device.hh \
            $(SRC)/host/GpuFeatureScorer.hh $(SRC)/gmm_hostio.hh include/rasr_gmm_io.h include/rasr_nn.h $(SRC)/nn_kernels.hh $(SRC)/gmm_shard.hh $(SRC)/gmm_scorer.hh

LIB       = $(LIBDIR)/librasr_gmm.so
OBJS      = $(BUILD)/gmm_kernels_i8.o $(BUILD)/gmm_kernels_f32.o $(BUILD)/gmm_kernels_split.o $(BUILD)/gmm_api.o $(BUILD)/gmm_prepare.o \
            $(BUILD)/GpuFeatureScorer.o $(BUILD)/MixtureSetFile.o $(BUILD)/MixtureSetEstimatorFile.o $(BUILD)/nn_kernels.o $(BUILD)/nn_api.o \
            $(BUILD)/gmm_kernels_presel.o $(BUILD)/gmm_presel.o $(BUILD)/gmm_kernels_shard.o $(BUILD)/gmm_hostio.o \
            $(BUILD)/gmm_kernels_direct.o $(BUILD)/gmm_kernels_layout.o $(BUILD)/gmm_shard.o $(BUILD)/gmm_kernels_pairs.o \
            $(BUILD)/gmm_create.o $(BUILD)/gmm_score.o $(BUILD)/gmm_hostcall.o $(BUILD)/gmm_group.o \
            $(BUILD)/gmm_kernels_accum.o $(BUILD)/gmm_estimator.o $(BUILD)/gmm_kernels_posterior.o \
            $(BUILD)/gmm_kernels_state.o $(BUILD)/gmm_state.o \
            $(BUILD)/gmm_kernels_keyed.o $(BUILD)/gmm_pairaccum.o $(BUILD)/PairTopology.o \
            $(BUILD)/gmm_kernels_adapt.o $(BUILD)/gmm_adapt.o $(BUILD)/AffineTransformEstimate.o \
            $(BUILD)/gmm_kernels_mllr.o $(BUILD)/gmm_mllr.o $(BUILD)/MllrEstimate.o \
            $(BUILD)/gmm_kernels_align.o $(BUILD)/gmm_kernels_align_posterior.o $(BUILD)/gmm_align.o $(BUILD)/AlignGraph.o
# the core of the handles that accumulate pairs (gmm_pairaccum.hh names the chunk constants of both adaptation headers)
PAIR_HDRS = $(SRC)/gmm_pairaccum.hh $(SRC)/host/PairTopology.hh $(SRC)/gmm_estimator.hh include/rasr_gmm_estimator.h \
            include/rasr_gmm_adaptation.h include/rasr_gmm_mllr.h
# include/rasr_gmm_estimator.h: the units behind it depend on these besides HDRS
EST_HDRS  = $(PAIR_HDRS)
# include/rasr_gmm_adaptation.h: the units behind it depend on these besides HDRS
ADAPT_HDRS = $(PAIR_HDRS) $(SRC)/gmm_adapt.hh
# include/rasr_gmm_mllr.h: the units behind it depend on these besides HDRS
MLLR_HDRS = $(PAIR_HDRS) $(SRC)/gmm_mllr.hh
# include/rasr_gmm_align.h: the units behind it depend on these (the kernel unit on nothing else)
ALIGN_HDRS = include/rasr_gmm_align.h include/rasr_gmm.h $(SRC)/gmm_align.hh $(SRC)/gmm_align_step.hh \
             $(SRC)/host/AlignGraph.hh
DRIVER    = $(BUILD)/tests/feature_scorer_driver

REFSORT   = $(BUILD)/tests/refsort_test
CLASSLAYOUT = $(BUILD)/tests/class_layout_test
ESTCOMBINE = $(BUILD)/tests/estimator_combine_test
AFFINEEST = $(BUILD)/tests/affine_estimate_test
EBWEST   = $(BUILD)/tests/ebw_estimate_test
MLLREST  = $(BUILD)/tests/mllr_estimate_test
PAIRTOPO = $(BUILD)/tests/pair_topology_test
ALIGNGRAPH = $(BUILD)/tests/align_graph_test
ALIGNPOSTGRAPH = $(BUILD)/tests/align_posterior_graph_test

all: $(LIB) $(DRIVER) $(REFSORT) $(CLASSLAYOUT) $(ESTCOMBINE) $(AFFINEEST) $(EBWEST) $(MLLREST) $(PAIRTOPO) $(ALIGNGRAPH) $(ALIGNPOSTGRAPH) oracle reference-scorers check-integration

$(BUILD)/gmm_kernels_i8.o: $(SRC)/gmm_kernels_i8.hip $(HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) $(I8FLAGS) -c $< -o $@

$(BUILD)/gmm_kernels_f32.o: $(SRC)/gmm_kernels_f32.hip $(HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) $(F32FLAGS) -c $< -o $@

$(BUILD)/gmm_kernels_split.o: $(SRC)/gmm_kernels_split.hip $(HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) $(SPLITFLAGS) -c $< -o $@

# density preselection: clustering assignment + per-frame cluster selection (std::sort replay)
$(BUILD)/gmm_kernels_presel.o: $(SRC)/gmm_kernels_presel.hip $(SRC)/gmm_refsort.hh $(HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# reference-order float scorers (GMM_FLAG_REFERENCE_ORDER): scalar f32 ops in the reference's order
# (no SLP packing into v_pk_*_f32, which issue at a third of the scalar VOP2 rate)
$(BUILD)/gmm_kernels_direct.o: $(SRC)/gmm_kernels_direct.hip $(HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) -fno-slp-vectorize -c $< -o $@

# sparse best densities of (frame, mixture) pairs (gmm_best_density_pairs): the reference's scalar order
$(BUILD)/gmm_kernels_pairs.o: $(SRC)/gmm_kernels_pairs.hip $(HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) -fno-slp-vectorize -c $< -o $@

# density posteriors of (frame, mixture) pairs and their Baum-Welch expansion (gmm_density_posteriors_pairs_*,
# gmm_estimator_accumulate_posteriors_*): the reference's scalar order, as gmm_kernels_pairs.  Not one of KERNEL_OBJS
$(BUILD)/gmm_kernels_posterior.o: $(SRC)/gmm_kernels_posterior.hip $(HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) -fno-slp-vectorize -c $< -o $@

# state posteriors over a score table (gmm_state_posteriors_*): f64 in a fixed order, every operation an _rn intrinsic.
# Not one of KERNEL_OBJS
$(BUILD)/gmm_kernels_state.o: $(SRC)/gmm_kernels_state.hip $(HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# maximum-likelihood and joint numerator / denominator accumulation (gmm_estimator_accumulate_*,
# gmm_estimator_accumulate_discriminative_*): resolve, inverted indexes (rocPRIM radix sort), ordered f64 sums with one
# or two chains per lane.  Not one of KERNEL_OBJS: gmm_kernel_id names the scoring kernels the PMC summaries measure
$(BUILD)/gmm_kernels_accum.o: $(SRC)/gmm_kernels_accum.hip $(EST_HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(BUILD)/gmm_estimator.o: $(SRC)/gmm_estimator.cc $(HDRS) $(EST_HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HOSTFLAGS) -c $< -o $@

# the shared core (gmm_pairaccum.hh): checks, staging and call shapes of the estimator, affine and MLLR handles; the
# keyed handles' resolve / index / combine passes, built with gmm_kernels_adapt's flags.  Not one of KERNEL_OBJS
$(BUILD)/gmm_kernels_keyed.o: $(SRC)/gmm_kernels_keyed.hip $(HDRS) $(PAIR_HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(BUILD)/gmm_pairaccum.o: $(SRC)/gmm_pairaccum.cc $(HDRS) $(PAIR_HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HOSTFLAGS) -c $< -o $@

$(BUILD)/PairTopology.o: $(SRC)/host/PairTopology.cc $(SRC)/host/PairTopology.hh include/rasr_gmm.h
	@mkdir -p $(BUILD)
	g++ $(HOSTFLAGS) -c $< -o $@

# affine feature transform (CMLLR) accumulation per speaker key (gmm_affine_accumulate_*): the pieces'
# ordered f64 sums with a correctly rounded division per G term.  Not one of KERNEL_OBJS
$(BUILD)/gmm_kernels_adapt.o: $(SRC)/gmm_kernels_adapt.hip $(HDRS) $(ADAPT_HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(BUILD)/gmm_adapt.o: $(SRC)/gmm_adapt.cc $(HDRS) $(ADAPT_HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HOSTFLAGS) -c $< -o $@

$(BUILD)/AffineTransformEstimate.o: $(SRC)/host/AffineTransformEstimate.cc include/rasr_gmm.h include/rasr_gmm_adaptation.h
	@mkdir -p $(BUILD)
	g++ $(HOSTFLAGS) -c $< -o $@

# MLLR mean transform accumulation per (speaker key, regression leaf) (gmm_mllr_accumulate_*): the pieces'
# ordered f64 sums; gmm_kernels_adapt's flags.  Not one of KERNEL_OBJS
$(BUILD)/gmm_kernels_mllr.o: $(SRC)/gmm_kernels_mllr.hip $(HDRS) $(MLLR_HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(BUILD)/gmm_mllr.o: $(SRC)/gmm_mllr.cc $(HDRS) $(MLLR_HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HOSTFLAGS) -c $< -o $@

$(BUILD)/MllrEstimate.o: $(SRC)/host/MllrEstimate.cc include/rasr_gmm.h include/rasr_gmm_mllr.h
	@mkdir -p $(BUILD)
	g++ $(HOSTFLAGS) -c $< -o $@

# Viterbi alignment over a score table (gmm_aligner_*): one workgroup per segment, f32 additions and comparisons only,
# every one an _rn intrinsic.  Not one of KERNEL_OBJS
$(BUILD)/gmm_kernels_align.o: $(SRC)/gmm_kernels_align.hip $(ALIGN_HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# Baum-Welch alignment (gmm_aligner_posteriors_*): the f32 search, the f64 potentials and the per-frame items, every
# add, subtract, multiply and divide an _rn intrinsic; exp and log1p are the device library's f64 functions
$(BUILD)/gmm_kernels_align_posterior.o: $(SRC)/gmm_kernels_align_posterior.hip $(ALIGN_HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(BUILD)/gmm_align.o: $(SRC)/gmm_align.cc $(HDRS) $(ALIGN_HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HOSTFLAGS) -c $< -o $@

$(BUILD)/AlignGraph.o: $(SRC)/host/AlignGraph.cc $(SRC)/host/AlignGraph.hh include/rasr_gmm.h include/rasr_gmm_align.h
	@mkdir -p $(BUILD)
	g++ $(HOSTFLAGS) -c $< -o $@

# density-sharded exchange keys (BASELINE config 4)
$(BUILD)/gmm_kernels_shard.o: $(SRC)/gmm_kernels_shard.hip $(HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# frame-major host tables (gmm_score_host_ring with GMM_HOST_FRAME_MAJOR)
$(BUILD)/gmm_kernels_layout.o: $(SRC)/gmm_kernels_layout.hip $(HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(BUILD)/gmm_presel.o: $(SRC)/gmm_presel.cc $(SRC)/gmm_presel.hh $(HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HOSTFLAGS) -c $< -o $@

# hybrid-DNN scorer (include/rasr_nn.h): bf16 MFMA GEMM per layer
$(BUILD)/nn_kernels.o: $(SRC)/nn_kernels.hip $(HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(BUILD)/nn_api.o: $(SRC)/nn_api.cc $(HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HOSTFLAGS) -c $< -o $@

# identity of the device code: a hash of the gfx950 code objects of the GMM scorer kernels (the kernels the PMC
# summaries profiles/pmc_*.json measure), so a summary stays matched to the ISA it was collected on -- a source
# edit that leaves the code unchanged keeps the id, any code change gives a new one; bench.py uses a summary
# only for the kernels it was measured on
BUNDLER  ?= $(ROCM_PATH)/lib/llvm/bin/clang-offload-bundler
KERNEL_OBJS = $(BUILD)/gmm_kernels_i8.o $(BUILD)/gmm_kernels_f32.o $(BUILD)/gmm_kernels_split.o
$(BUILD)/kernel_id.h: $(KERNEL_OBJS)
	@for o in $(KERNEL_OBJS); do objcopy -O binary --only-section=.hip_fatbin $$o $$o.fatbin && \
	     $(BUNDLER) --unbundle --type=o --input=$$o.fatbin --targets=hipv4-amdgcn-amd-amdhsa--$(ARCH) \
	     --output=$$o.$(ARCH) || exit 1; done
	@echo "#define GMM_KERNEL_ID \"$$(cat $(addsuffix .$(ARCH),$(KERNEL_OBJS)) | sha256sum | cut -c1-16)\"" > $@

$(BUILD)/gmm_api.o: $(SRC)/gmm_api.cc $(HDRS) $(BUILD)/kernel_id.h
	@mkdir -p $(BUILD)
	$(HIPCC) $(HOSTFLAGS) -I$(BUILD) -c $< -o $@

# the other units behind include/rasr_gmm.h (gmm_scorer.hh lists them)
$(BUILD)/gmm_create.o $(BUILD)/gmm_score.o $(BUILD)/gmm_hostcall.o $(BUILD)/gmm_group.o $(BUILD)/gmm_state.o: $(BUILD)/%.o: $(SRC)/%.cc $(HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HOSTFLAGS) -c $< -o $@

$(BUILD)/gmm_hostio.o: $(SRC)/gmm_hostio.cc $(HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HOSTFLAGS) -pthread -c $< -o $@

# density shard plan (gmm_scorer_create_sharded, gmm_density_shard_plan)
$(BUILD)/gmm_shard.o: $(SRC)/gmm_shard.cc $(HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HOSTFLAGS) -c $< -o $@

$(BUILD)/gmm_prepare.o: $(SRC)/gmm_prepare.cc $(HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HOSTFLAGS) -c $< -o $@

$(BUILD)/GpuFeatureScorer.o: $(SRC)/host/GpuFeatureScorer.cc $(HDRS)
	@mkdir -p $(BUILD)
	g++ $(HOSTFLAGS) -c $< -o $@

$(BUILD)/MixtureSetFile.o: $(SRC)/host/MixtureSetFile.cc $(HDRS)
	@mkdir -p $(BUILD)
	g++ $(HOSTFLAGS) -c $< -o $@

$(BUILD)/MixtureSetEstimatorFile.o: $(SRC)/host/MixtureSetEstimatorFile.cc $(HDRS) $(EST_HDRS)
	@mkdir -p $(BUILD)
	g++ $(HOSTFLAGS) -c $< -o $@

$(LIB): $(OBJS)
	@mkdir -p $(LIBDIR)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJS) -lz -pthread -ldl

# host check of the score-only layout against the SCORE_ONLY kernel's arithmetic (no GPU)
$(CLASSLAYOUT): tests/cpp/class_layout_test.cc $(BUILD)/gmm_prepare.o $(HDRS)
	@mkdir -p $(BUILD)/tests
	$(HIPCC) $(HOSTFLAGS) -c $< -o $@.o
	$(HIPCC) -o $@ $@.o $(BUILD)/gmm_prepare.o

# host pin of the GPU std::sort replay (gmm_refsort.hh) against this image's std::sort
$(REFSORT): tests/cpp/refsort_test.cc $(SRC)/gmm_refsort.hh
	@mkdir -p $(BUILD)/tests
	g++ -std=c++17 -O2 -Wall -o $@ $<

# host check of gmm_estimator_combine and the estimator file writer (no GPU, no HIP): the two file units alone
$(ESTCOMBINE): tests/cpp/estimator_combine_test.cc $(SRC)/host/MixtureSetEstimatorFile.cc $(SRC)/host/MixtureSetFile.cc \
               $(HDRS) $(EST_HDRS)
	@mkdir -p $(BUILD)/tests
	g++ $(HOSTFLAGS) $(ESTCOMBINE_FLAGS) -o $@ $< $(SRC)/host/MixtureSetEstimatorFile.cc $(SRC)/host/MixtureSetFile.cc -lz

# host check of the discriminative estimator file writer, gmm_estimator_combine_discriminative and
# gmm_estimator_estimate_ebw (no GPU, no HIP): the two file units alone
$(EBWEST): tests/cpp/ebw_estimate_test.cc $(SRC)/host/MixtureSetEstimatorFile.cc $(SRC)/host/MixtureSetFile.cc \
            $(HDRS) $(EST_HDRS)
	@mkdir -p $(BUILD)/tests
	g++ $(HOSTFLAGS) $(EBWEST_FLAGS) -o $@ $< $(SRC)/host/MixtureSetEstimatorFile.cc $(SRC)/host/MixtureSetFile.cc -lz

# host check of gmm_affine_estimate (no GPU, no HIP): the estimate unit alone
$(AFFINEEST): tests/cpp/affine_estimate_test.cc $(SRC)/host/AffineTransformEstimate.cc include/rasr_gmm.h include/rasr_gmm_adaptation.h
	@mkdir -p $(BUILD)/tests
	g++ $(HOSTFLAGS) $(AFFINEEST_FLAGS) -o $@ $< $(SRC)/host/AffineTransformEstimate.cc

# host check of gmm_mllr_estimate and gmm_mllr_adapt_means (no GPU, no HIP): the estimate unit alone
$(MLLREST): tests/cpp/mllr_estimate_test.cc $(SRC)/host/MllrEstimate.cc include/rasr_gmm.h include/rasr_gmm_mllr.h
	@mkdir -p $(BUILD)/tests
	g++ $(HOSTFLAGS) $(MLLREST_FLAGS) -o $@ $< $(SRC)/host/MllrEstimate.cc

# host check of the topology validation and expansion that the three accumulating handles share (no GPU, no HIP)
$(PAIRTOPO): tests/cpp/pair_topology_test.cc $(SRC)/host/PairTopology.cc $(SRC)/host/PairTopology.hh include/rasr_gmm.h
	@mkdir -p $(BUILD)/tests
	g++ $(HOSTFLAGS) $(PAIRTOPO_FLAGS) -o $@ $< $(SRC)/host/PairTopology.cc

# host check of the alignment graphs' validation and incoming-arc lists (no GPU, no HIP): the graph unit alone
ALIGNGRAPH_SRCS = tests/cpp/align_graph_test.cc $(SRC)/host/AlignGraph.cc
ALIGNGRAPH_DEPS = $(ALIGNGRAPH_SRCS) $(SRC)/host/AlignGraph.hh include/rasr_gmm.h include/rasr_gmm_align.h
$(ALIGNGRAPH): $(ALIGNGRAPH_DEPS)
	@mkdir -p $(BUILD)/tests
	g++ $(HOSTFLAGS) -o $@ $(ALIGNGRAPH_SRCS)

# the same program under the address and undefined-behaviour sanitizers, built and run on the CPU
$(ALIGNGRAPH)_san: $(ALIGNGRAPH_DEPS)
	@mkdir -p $(BUILD)/tests
	g++ $(HOSTFLAGS) -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $(ALIGNGRAPH_SRCS)
check-align-graph: $(ALIGNGRAPH)_san
	$(ALIGNGRAPH)_san

# host check of the mixture groups and the column order that the Baum-Welch call reads (no GPU, no HIP)
ALIGNPOSTGRAPH_SRCS = tests/cpp/align_posterior_graph_test.cc $(SRC)/host/AlignGraph.cc
ALIGNPOSTGRAPH_DEPS = $(ALIGNPOSTGRAPH_SRCS) $(SRC)/host/AlignGraph.hh include/rasr_gmm.h include/rasr_gmm_align.h
$(ALIGNPOSTGRAPH): $(ALIGNPOSTGRAPH_DEPS)
	@mkdir -p $(BUILD)/tests
	g++ $(HOSTFLAGS) -o $@ $(ALIGNPOSTGRAPH_SRCS)
	$@
$(ALIGNPOSTGRAPH)_san: $(ALIGNPOSTGRAPH_DEPS)
	@mkdir -p $(BUILD)/tests
	g++ $(HOSTFLAGS) -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $(ALIGNPOSTGRAPH_SRCS)
check-align-posterior-graph: $(ALIGNPOSTGRAPH)_san
	$(ALIGNPOSTGRAPH)_san

$(DRIVER): tests/cpp/feature_scorer_driver.cc $(LIB) $(HDRS)
	@mkdir -p $(BUILD)/tests
	g++ $(HOSTFLAGS) -o $@ $< -L$(LIBDIR) -lrasr_gmm -Wl,-rpath,'$$ORIGIN/../../$(LIBDIR)'

oracle:
	$(MAKE) -C oracle

# The reference's OWN scorers as a stand-alone executable, oracle/_ref/ref_scorers (test infrastructure: what the
# oracle is pinned to, tests/test_reference_pin.py; recipe and flags in oracle/ref/Makefile).  Built where
# $(RASR_REF)/src exists; elsewhere (the GPU box) nothing happens and an executable already there stays.  A
# failure here never fails the build: the tests that need the executable then say why they skip.
RASR_REF ?= /root/reference
reference-scorers:
	@$(MAKE) -s -C oracle/ref RASR_REF=$(RASR_REF) all || \
	    echo "reference-scorers: build failed; the live reference pin will skip (fixtures under tests/golden/ref still run)"

# The RASR-side adapter (integration/rasr/Mm/GpuFeatureScorer.{hh,cc}) compiled -fsyntax-only against the
# reference's own headers with the reference's flags (config/cc-gcc.make:26-29).  Core/Utility.hh includes the
# make-generated Modules.hh, so a one-line stand-in (MODULE_MM_BATCH, as src/Mm/Makefile:70-75 builds it) is
# written under build/ for this check only; it pins no parity and nothing is linked.  Skipped where the
# reference tree is absent (the GPU box).
RASR_SRC ?= /root/reference/src
check-integration: integration/rasr/Mm/GpuFeatureScorer.cc integration/rasr/Mm/GpuFeatureScorer.hh $(SRC)/host/GpuFeatureScorer.hh \
                   integration/rasr/Nn/GpuBatchFeatureScorer.cc integration/rasr/Nn/GpuBatchFeatureScorer.hh \
                   integration/rasr/Nn/GpuBatchFeatureScorerNetwork.cc include/rasr_nn.h
	@if [ -d "$(RASR_SRC)/Mm" ]; then \
	    mkdir -p $(BUILD)/rasr_check && printf '#pragma once\n#define MODULE_MM_BATCH\n' > $(BUILD)/rasr_check/Modules.hh && \
	    g++ -std=gnu++0x -fsyntax-only -funsigned-char -fno-exceptions -Wall -DPROC_x86_64 -DOS_linux \
	        -DARCH_linux_x86_64 -D_GNU_SOURCE -I$(BUILD)/rasr_check -I$(RASR_SRC) -I/usr/include/libxml2 -Iinclude \
	        -I$(SRC) integration/rasr/Mm/GpuFeatureScorer.cc && \
	    g++ -std=gnu++0x -fsyntax-only -funsigned-char -fno-exceptions -Wall -DPROC_x86_64 -DOS_linux \
	        -DARCH_linux_x86_64 -D_GNU_SOURCE -I$(BUILD)/rasr_check -I$(RASR_SRC) -I/usr/include/libxml2 \
	        -Iinclude integration/rasr/Nn/GpuBatchFeatureScorer.cc && \
	    echo "check-integration: adapters compile against $(RASR_SRC) (Mm; Nn protocol unit -- its network unit" \
	         "includes Math/Blas.hh -> <cblas.h>, absent from this image, and is not checked)"; \
	else echo "check-integration: $(RASR_SRC) absent, skipped"; fi

# The RASR-side adapter LINKED and RUN on the CPU (test infrastructure): integration/rasr/Mm/GpuFeatureScorer.cc and
# the real host classes (rasr_amd/csrc/host/GpuFeatureScorer.cc) inside test doubles of RASR's plugin machinery
# (tests/rasr_harness/include, see its README), over an oracle-backed stand-in of the C-ABI; driven through the
# factory, FeatureScorerScaling, the recognizer and the score-dump call sequences (tests/rasr_harness/harness.cc).
HARNESS = $(BUILD)/tests/rasr_adapter_harness
$(HARNESS): tests/rasr_harness/harness.cc tests/rasr_harness/gmm_standin.cc integration/rasr/Mm/GpuFeatureScorer.cc \
            integration/rasr/Mm/GpuFeatureScorer.hh $(SRC)/host/GpuFeatureScorer.cc $(SRC)/host/GpuFeatureScorer.hh \
            $(wildcard tests/rasr_harness/include/*/*.hh) | oracle
	@mkdir -p $(BUILD)/tests
	g++ -std=c++17 -O1 -Wall -Wno-unused-variable -Itests/rasr_harness/include -Iinclude -I$(SRC) -o $@ \
	    tests/rasr_harness/harness.cc tests/rasr_harness/gmm_standin.cc integration/rasr/Mm/GpuFeatureScorer.cc \
	    $(SRC)/host/GpuFeatureScorer.cc -Loracle/_build -lgmm_oracle -Wl,-rpath,'$$ORIGIN/../../oracle/_build' -lm -pthread

# The hybrid-DNN adapter (all three integration/rasr/Nn files) linked and run the same way: test doubles of the Nn
# network, prior and class-label classes (tests/rasr_harness/include/Nn), over an f32 stand-in of the NN C-ABI (CPU)
# or the product library (GPU build, run by tests/test_nn_integration.py -m gpu)
NN_ADAPTER = integration/rasr/Nn/GpuBatchFeatureScorer.cc integration/rasr/Nn/GpuBatchFeatureScorerNetwork.cc
NN_HARNESS_DEPS = tests/rasr_harness/nn_harness.cc $(NN_ADAPTER) integration/rasr/Nn/GpuBatchFeatureScorer.hh \
                  include/rasr_nn.h $(wildcard tests/rasr_harness/include/*/*.hh)
NN_HARNESS_FLAGS = -std=c++17 -O1 -Wall -Wno-unused-variable -Itests/rasr_harness/include -Itests/rasr_harness/include/Nn -Iinclude
NN_HARNESS = $(BUILD)/tests/rasr_nn_harness
$(NN_HARNESS): $(NN_HARNESS_DEPS) tests/rasr_harness/nn_standin.cc
	@mkdir -p $(BUILD)/tests
	g++ $(NN_HARNESS_FLAGS) -o $@ tests/rasr_harness/nn_harness.cc $(NN_ADAPTER) tests/rasr_harness/nn_standin.cc -lm
NN_HARNESS_GPU = $(BUILD)/tests/rasr_nn_harness_gpu
$(NN_HARNESS_GPU): $(NN_HARNESS_DEPS) $(LIB)
	@mkdir -p $(BUILD)/tests
	g++ $(NN_HARNESS_FLAGS) -DHARNESS_PRODUCT -o $@ tests/rasr_harness/nn_harness.cc $(NN_ADAPTER) \
	    -L$(LIBDIR) -lrasr_gmm -Wl,-rpath,'$$ORIGIN/../../$(LIBDIR)' -lm -pthread

check-integration-link: $(HARNESS) $(NN_HARNESS)
	$(HARNESS)

# The same adapter + harness over the PRODUCT library (librasr_gmm.so: the HIP kernels and the host classes inside
# it); the oracle is linked as the checker.  Built here, run on the GPU by tests/test_integration.py (-m gpu).
HARNESS_GPU = $(BUILD)/tests/rasr_adapter_harness_gpu
$(HARNESS_GPU): tests/rasr_harness/harness.cc integration/rasr/Mm/GpuFeatureScorer.cc integration/rasr/Mm/GpuFeatureScorer.hh \
                $(SRC)/host/GpuFeatureScorer.hh $(wildcard tests/rasr_harness/include/*/*.hh) $(LIB) | oracle
	@mkdir -p $(BUILD)/tests
	g++ -std=c++17 -O1 -Wall -Wno-unused-variable -DHARNESS_PRODUCT -Itests/rasr_harness/include -Iinclude -I$(SRC) -o $@ \
	    tests/rasr_harness/harness.cc integration/rasr/Mm/GpuFeatureScorer.cc \
	    -L$(LIBDIR) -lrasr_gmm -Loracle/_build -lgmm_oracle \
	    -Wl,-rpath,'$$ORIGIN/../../$(LIBDIR)' -Wl,-rpath,'$$ORIGIN/../../oracle/_build' -lm -pthread

# the harness binaries (variables defined above): built with everything else, so they travel to the GPU box
all: $(HARNESS_GPU) $(NN_HARNESS) $(NN_HARNESS_GPU)

clean:
	rm -rf $(BUILD) $(LIBDIR)
	$(MAKE) -C oracle clean

# make -s print-VAR: a variable's value (scripts/build_variants.sh takes the per-TU kernel flags from here)
print-%:
	@echo '$($*)'

.PHONY: all oracle reference-scorers clean check-integration check-integration-link check-align-graph check-align-posterior-graph
