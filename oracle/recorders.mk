# TEST INFRASTRUCTURE -- builds and runs the golden recorders, tests/golden/record_*_reference.cpp, never the product.
# Included from oracle/Makefile (HERE, REPO, REF, OUT, OBJ, CXX).  Only possible where $(REF) exists; outputs only into oracle/_ref/.
#
#   make recorders       -> the 14 programs under oracle/_ref/obj/recorders/
#   make rerecord        -> runs those that make their own inputs (all but pusch_processor and pusch_csi2, which read grids a
#                           GPU wrote: `python tests/test_pusch_processor.py DIR`, `python tests/test_pusch_csi2.py DIR`; they
#                           run too when PUSCH_PROC_INPUTS=DIR, PUSCH_CSI2_INPUTS=DIR name such directories); recordings go to
#                           oracle/_ref/recorded/.  The SRS run alone takes minutes; give make -j (at most 16).
#   make rerecord-check  -> cmp of every recorded file against the one of its name in tests/golden/
#
# The reference's translation units are named by path and compiled where they lie, once per flag set ("flavour"); a recorder
# links the objects of its own list.  Why a flavour is what it is:
#   nc      -ffp-contract=off: a recording holds what the source says, operation by operation; g++'s default would fuse a * b + c
#           wherever the target has a fused multiply-add (the SRS estimator's phase index n * ps + offset, for one).
#   avx2    the AVX2 build is the one the library's LDPC, demapper and compression kernels are pinned to.
#   nc (without avx2), for channel_equalizer_generic_impl.cpp of pusch_tp and of the processors' archive alone: the library's
#           equaliser is pinned to the reference's scalar loops with exact division (include/mi355_nrphy.h,
#           nrphy_channel_equalize), and under __AVX2__ equalize_zf_1xn.h:65-126 and equalize_zf_2xn.h:79-179 replace them, for
#           the first floor(n / 8) * 8 RE, by a form with an approximate reciprocal (srsran_simd_f_rcp, about 1e-4 off).
#   avx512nc  the *avx512* files and crc_calculator_clmul_impl.cpp, which the factories name but no recorder ever selects.

REC      := $(OBJ)/recorders
GOLDEN   := $(REPO)/tests/golden
RECORDED := $(OUT)/recorded
REC_BASE := -std=c++17 -O2 -DNDEBUG -w -I$(REF)/include -I$(REF)/external/fmt/include -I$(REF)/external -I$(REF)

FLAGS_plain    :=
FLAGS_avx2     := -mavx2 -mfma
FLAGS_nc       := -ffp-contract=off
FLAGS_avx2nc   := -mavx2 -mfma -ffp-contract=off
FLAGS_avx512nc := $(FLAGS_avx2nc) -mavx512f -mavx512bw -mavx512vl -mavx512dq -mavx512vbmi -mpclmul -msse4.1
FLAVOURS       := plain avx2 nc avx2nc avx512nc

define flavour_rule
$(REC)/$(1)/%.o: $(REF)/%
	@mkdir -p $$(dir $$@)
	$(CXX) $(REC_BASE) $(FLAGS_$(1)) -c $$< -o $$@
endef
$(foreach f,$(FLAVOURS),$(eval $(call flavour_rule,$(f))))

U      := lib/phy/upper
FMT    := external/fmt/src/format.cc external/fmt/src/os.cc
SRSLOG := lib/srslog/srslog.cpp lib/srslog/backend_worker.cpp lib/srslog/event_trace.cpp \
          lib/srslog/formatters/json_formatter.cpp lib/srslog/formatters/text_formatter.cpp
SRSVEC := $(patsubst $(REF)/%,%,$(wildcard $(REF)/lib/srsvec/*.cpp))
OFH_COMPRESSION := lib/ofh/compression/iq_compression_none_impl.cpp lib/ofh/compression/iq_compression_bfp_impl.cpp \
                   lib/ofh/compression/compressed_prb_packer.cpp lib/ofh/compression/compressed_prb_unpacker.cpp
CHEST  := $(U)/signal_processors/port_channel_estimator_average_impl.cpp $(U)/sequence_generators/pseudo_random_generator_impl.cpp \
          lib/phy/support/time_alignment_estimator/time_alignment_estimator_dft_impl.cpp \
          lib/phy/support/interpolator/interpolator_linear_impl.cpp lib/phy/generic_functions/dft_processor_generic_impl.cpp \
          lib/support/math_utils.cpp $(SRSVEC)

# ---- per recorder: its flavour, the reference sources it links, what its own translation unit needs besides ----
FLAVOUR_ulsch_demultiplex := avx2
SRCS_ulsch_demultiplex    := $(U)/channel_processors/pusch/ulsch_demultiplex_impl.cpp $(U)/sequence_generators/pseudo_random_generator_impl.cpp \
                             $(U)/log_likelihood_ratio.cpp lib/srsvec/bit.cpp lib/srsvec/compare.cpp lib/srsvec/aligned_vec.cpp $(FMT)
ARGS_ulsch_demultiplex    := $(GOLDEN)/ulsch_demultiplex_configs.json $(RECORDED)

FLAVOUR_uci := avx2
SRCS_uci    := $(U)/channel_processors/uci/uci_decoder_impl.cpp $(U)/channel_coding/short/short_block_detector_impl.cpp \
               $(U)/channel_coding/short/short_block_encoder_impl.cpp $(U)/channel_coding/polar/polar_code_impl.cpp \
               $(U)/channel_coding/polar/polar_rate_dematcher_impl.cpp $(U)/channel_coding/polar/polar_decoder_impl.cpp \
               $(U)/channel_coding/polar/polar_deallocator_impl.cpp $(U)/channel_coding/polar/polar_encoder_impl.cpp \
               $(U)/channel_coding/polar/polar_allocator_impl.cpp $(U)/channel_coding/polar/polar_rate_matcher_impl.cpp \
               $(U)/channel_coding/crc_calculator_generic_impl.cpp $(U)/log_likelihood_ratio.cpp lib/srsvec/bit.cpp lib/srsvec/dot_prod.cpp \
               lib/srsvec/aligned_vec.cpp lib/srsvec/compare.cpp $(FMT)
ARGS_uci    := $(GOLDEN)/uci_decoder_configs.json $(RECORDED)

FLAVOUR_prach_demod := plain
SRCS_prach_demod    := lib/phy/lower/modulation/ofdm_prach_demodulator_impl.cpp lib/phy/generic_functions/dft_processor_generic_impl.cpp \
                       lib/ran/prach/prach_preamble_information.cpp lib/ran/prach/prach_frequency_mapping.cpp lib/srsvec/aligned_vec.cpp $(FMT)
ARGS_prach_demod    := $(GOLDEN)/prach_demod_configs.json $(RECORDED)

FLAVOUR_prach_detector := avx2
SRCS_prach_detector    := $(U)/channel_processors/prach_detector_generic_impl.cpp $(U)/channel_processors/prach_generator_impl.cpp \
                          lib/phy/generic_functions/dft_processor_generic_impl.cpp lib/ran/prach/prach_preamble_information.cpp \
                          lib/ran/prach/prach_cyclic_shifts.cpp lib/support/math_utils.cpp $(SRSVEC) $(FMT)
ARGS_prach_detector    := $(GOLDEN)/prach_detector_configs.json $(RECORDED)

FLAVOUR_pucch := avx2nc
SRCS_pucch    := $(U)/channel_processors/pucch_detector_format0.cpp $(U)/channel_processors/pucch_detector_format1.cpp \
                 $(U)/signal_processors/pucch/dmrs_pucch_processor_format1_impl.cpp $(U)/equalization/channel_equalizer_generic_impl.cpp \
                 $(U)/sequence_generators/low_papr_sequence_collection_impl.cpp $(U)/sequence_generators/low_papr_sequence_generator_impl.cpp \
                 $(CHEST) $(FMT)
ARGS_pucch    := $(GOLDEN)/pucch_configs.json $(RECORDED)

# The flags of pusch_chest are those of the processors' archive, so both recordings describe one build of the reference.
FLAVOUR_pusch_chest := avx2nc
SRCS_pusch_chest    := $(U)/signal_processors/dmrs_pusch_estimator_impl.cpp $(CHEST) $(FMT)
ARGS_pusch_chest    := $(GOLDEN)/pusch_chest_configs.json $(RECORDED)

FLAVOUR_srs := avx2nc
SRCS_srs    := $(U)/signal_processors/srs/srs_estimator_generic_impl.cpp $(U)/sequence_generators/low_papr_sequence_generator_impl.cpp \
               lib/phy/support/time_alignment_estimator/time_alignment_estimator_dft_impl.cpp \
               lib/phy/generic_functions/dft_processor_generic_impl.cpp lib/ran/srs/srs_information.cpp \
               lib/ran/srs/srs_bandwidth_configuration.cpp lib/support/math_utils.cpp lib/srsvec/prod.cpp lib/srsvec/add.cpp \
               lib/srsvec/sc_prod.cpp lib/srsvec/compare.cpp lib/srsvec/aligned_vec.cpp $(FMT)
ARGS_srs    := $(GOLDEN)/srs_configs.json $(RECORDED)

EQUALIZER_SCALAR  := $(REC)/nc/$(U)/equalization/channel_equalizer_generic_impl.cpp.o
FLAVOUR_pusch_tp := avx2nc
SRCS_pusch_tp    := $(U)/channel_processors/pusch/pusch_demodulator_impl.cpp $(U)/channel_modulation/demodulation_mapper_impl.cpp \
                    $(U)/channel_modulation/demodulation_mapper_qpsk.cpp $(U)/channel_modulation/demodulation_mapper_qam16.cpp \
                    $(U)/channel_modulation/demodulation_mapper_qam64.cpp $(U)/channel_modulation/demodulation_mapper_qam256.cpp \
                    $(U)/sequence_generators/pseudo_random_generator_impl.cpp $(U)/log_likelihood_ratio.cpp \
                    lib/phy/generic_functions/transform_precoding/transform_precoder_dft_impl.cpp lib/support/math_utils.cpp \
                    $(SRSVEC) $(FMT)
LINK_pusch_tp    := $(EQUALIZER_SCALAR)
ARGS_pusch_tp    := $(GOLDEN)/pusch_demodulator_configs.json $(RECORDED)

# PUCCH format 2: the flags of the processors' archive, and the scalar equaliser for the reason pusch_tp has it.
FLAVOUR_pf2 := avx2nc
SRCS_pf2    := $(filter-out $(FMT) lib/srsvec/%,$(SRCS_uci)) $(CHEST) \
               $(U)/signal_processors/pucch/dmrs_pucch_processor_format2_impl.cpp $(U)/channel_processors/pucch_demodulator_impl.cpp \
               $(U)/channel_modulation/demodulation_mapper_impl.cpp $(U)/channel_modulation/demodulation_mapper_qpsk.cpp \
               $(U)/channel_modulation/demodulation_mapper_qam16.cpp $(U)/channel_modulation/demodulation_mapper_qam64.cpp \
               $(U)/channel_modulation/demodulation_mapper_qam256.cpp $(FMT)
LINK_pf2    := $(EQUALIZER_SCALAR)
ARGS_pf2    := $(GOLDEN)/pf2_configs.json $(RECORDED)

OFH_RECEIVER_DOUBLES := -I$(REF)/tests/unittests/ofh/receiver

FLAVOUR_ofh_ul := plain
SRCS_ofh_ul    := $(OFH_COMPRESSION) lib/ofh/receiver/ofh_uplane_rx_symbol_data_flow_writer.cpp \
                  lib/ofh/receiver/ofh_uplane_prach_symbol_data_flow_writer.cpp lib/ran/prach/prach_frequency_mapping.cpp \
                  lib/ran/prach/prach_preamble_information.cpp lib/instrumentation/traces/ofh_traces.cpp lib/srsvec/conversion.cpp \
                  lib/srsvec/dot_prod.cpp lib/srsvec/aligned_vec.cpp $(SRSLOG) $(FMT)
OWN_ofh_ul     := $(OFH_RECEIVER_DOUBLES)
ARGS_ofh_ul    := $(RECORDED)

FLAVOUR_ofh_rx := plain
SRCS_ofh_rx    := lib/ofh/receiver/ofh_message_receiver.cpp lib/ofh/receiver/ofh_rx_window_checker.cpp \
                  lib/ofh/receiver/ofh_data_flow_uplane_uplink_data_impl.cpp lib/ofh/receiver/ofh_uplane_rx_symbol_data_flow_writer.cpp \
                  lib/ofh/receiver/ofh_uplane_rx_symbol_data_flow_notifier.cpp lib/ofh/ethernet/vlan_ethernet_frame_decoder_impl.cpp \
                  lib/ofh/ecpri/ecpri_packet_decoder_impl.cpp lib/ofh/serdes/ofh_uplane_message_decoder_impl.cpp \
                  lib/ofh/serdes/ofh_uplane_message_decoder_static_compression_impl.cpp \
                  lib/ofh/serdes/ofh_uplane_message_decoder_dynamic_compression_impl.cpp lib/ofh/compression/iq_decompressor_selector.cpp \
                  $(OFH_COMPRESSION) lib/ofh/compression/iq_compression_death_impl.cpp lib/instrumentation/traces/ofh_traces.cpp \
                  lib/srsvec/conversion.cpp lib/srsvec/dot_prod.cpp lib/srsvec/aligned_vec.cpp $(SRSLOG) $(FMT)
OWN_ofh_rx     := $(OFH_RECEIVER_DOUBLES)
ARGS_ofh_rx    := $(RECORDED)

# -fno-access-control is for one line of the recorder: the data flow's sequence generator always starts at 0, and the case with
# sequence identifiers 254, 255, 0 sets its counter.
FLAVOUR_ofh_dl := avx2
SRCS_ofh_dl    := lib/ofh/transmitter/ofh_data_flow_uplane_downlink_data_impl.cpp lib/ofh/transmitter/ofh_uplane_fragment_size_calculator.cpp \
                  lib/ofh/ethernet/vlan_ethernet_frame_builder_impl.cpp lib/ofh/ecpri/ecpri_packet_builder_impl.cpp \
                  lib/ofh/serdes/ofh_uplane_message_builder_impl.cpp lib/ofh/serdes/ofh_uplane_message_builder_static_compression_impl.cpp \
                  lib/ofh/serdes/ofh_uplane_message_builder_dynamic_compression_impl.cpp $(OFH_COMPRESSION) \
                  lib/ofh/compression/iq_compression_none_avx2.cpp lib/ofh/compression/iq_compression_bfp_avx2.cpp \
                  lib/instrumentation/traces/ofh_traces.cpp lib/srsvec/conversion.cpp lib/srsvec/aligned_vec.cpp $(SRSLOG) $(FMT)
OWN_ofh_dl     := -fno-access-control
ARGS_ofh_dl    := $(RECORDED)

# The two processor recorders link one archive: every .cpp under LIBREF_DIRS except what another architecture or a further
# library would need; the factories' file of the generic functions needs FFTW's header (the recorders bring a DFT factory).
LIBREF_DIRS := lib/phy/upper lib/phy/support lib/phy/generic_functions lib/srsvec lib/srslog lib/ran lib/support
rwildcard    = $(foreach d,$(wildcard $(1)/*),$(call rwildcard,$(d),$(2)) $(filter $(2),$(d)))
without      = $(foreach f,$(2),$(if $(findstring $(1),$(f)),,$(f)))
LIBREF_ALL  := $(patsubst $(REF)/%,%,$(foreach d,$(LIBREF_DIRS),$(call rwildcard,$(REF)/$(d),%.cpp)))
LIBREF_ALL  := $(call without,neon,$(call without,fftw,$(LIBREF_ALL)))
LIBREF_ALL  := $(call without,lib/support/network/,$(call without,lib/support/build_info/,$(call without,lib/support/version/,$(LIBREF_ALL))))
LIBREF_ALL  := $(filter-out lib/phy/generic_functions/generic_functions_factories.cpp lib/support/config_yaml.cpp,$(LIBREF_ALL)) $(FMT)
LIBREF_NC       := $(U)/equalization/channel_equalizer_generic_impl.cpp
LIBREF_AVX512NC := $(foreach f,$(LIBREF_ALL),$(if $(findstring avx512,$(f)),$(f))) $(U)/channel_coding/crc_calculator_clmul_impl.cpp
LIBREF_AVX2NC   := $(filter-out $(LIBREF_NC) $(LIBREF_AVX512NC),$(LIBREF_ALL))
LIBREF_OBJS     := $(patsubst %,$(REC)/avx2nc/%.o,$(LIBREF_AVX2NC)) $(patsubst %,$(REC)/nc/%.o,$(LIBREF_NC)) \
                   $(patsubst %,$(REC)/avx512nc/%.o,$(LIBREF_AVX512NC))

$(REC)/libref.a: $(LIBREF_OBJS)
	rm -f $@
	ar rcs $@ $^

FLAVOUR_pusch_processor := avx2nc
LINK_pusch_processor    := $(REC)/libref.a
ARGS_pusch_processor    := $(PUSCH_PROC_INPUTS) $(RECORDED)
FLAVOUR_pusch_csi2      := avx2nc
LINK_pusch_csi2         := $(REC)/libref.a
ARGS_pusch_csi2         := $(PUSCH_CSI2_INPUTS) $(RECORDED)

SELF_CONTAINED := ulsch_demultiplex uci prach_demod prach_detector pucch pf2 pusch_chest srs pusch_tp ofh_ul ofh_rx ofh_dl
RECORDERS      := $(SELF_CONTAINED) pusch_processor pusch_csi2
RERECORDED     := $(SELF_CONTAINED) $(if $(PUSCH_PROC_INPUTS),pusch_processor) $(if $(PUSCH_CSI2_INPUTS),pusch_csi2)

define recorder_rule
$(REC)/record_$(1)_reference: $(GOLDEN)/record_$(1)_reference.cpp $(wildcard $(GOLDEN)/recorder_*.h) \
                              $(patsubst %,$(REC)/$(FLAVOUR_$(1))/%.o,$(SRCS_$(1))) $(LINK_$(1))
	@mkdir -p $$(dir $$@)
	$(CXX) $(REC_BASE) $(FLAGS_$(FLAVOUR_$(1))) $(OWN_$(1)) $$(filter-out %.h,$$^) -lpthread -o $$@

.PHONY: rerecord-$(1)
rerecord-$(1): $(REC)/record_$(1)_reference
	@mkdir -p $(RECORDED)
	@start=$$$$(date +%s) && $$< $(ARGS_$(1)) && echo "record_$(1)_reference: $$$$(( $$$$(date +%s) - start )) s"
endef
$(foreach r,$(RECORDERS),$(eval $(call recorder_rule,$(r))))

.PHONY: recorders rerecord rerecord-check
recorders: $(patsubst %,$(REC)/record_%_reference,$(RECORDERS))

rerecord: $(addprefix rerecord-,$(RERECORDED))

rerecord-prach_demod: rerecord-prach_demod-tables
.PHONY: rerecord-prach_demod-tables
rerecord-prach_demod-tables: $(REC)/record_prach_demod_reference
	@mkdir -p $(RECORDED)
	$< --tables > $(RECORDED)/prach_demod_tables.json

rerecord-check: rerecord
	@bad=0; for f in $(RECORDED)/*; do n=$$(basename $$f); \
	  if [ -f $(GOLDEN)/$$n ] && cmp -s $$f $(GOLDEN)/$$n; then echo "$$n same"; else echo "$$n DIFFERS"; bad=1; fi; \
	done; exit $$bad
