# Top-level build: the HIP engine (gfx950 only) and the CPU oracle (test infrastructure).
HIPCC ?= /opt/rocm/bin/hipcc
PKG := u96-slam_amd
CSRC := $(PKG)/csrc
LIB := $(PKG)/lib/libsbm_hip.so
# --offload-compress: the device code objects are stored compressed (10.5 MB -> 2.3 MB; ~4 ms of decompression at first use)
HIPFLAGS ?= --offload-arch=gfx950 --offload-compress -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -Wno-unused-value -Wno-unused-result
SRCS := $(CSRC)/sbm_api.hip $(CSRC)/sbm_host.hip $(CSRC)/sbm_prefilter.hip $(CSRC)/sbm_sad_generic.hip $(CSRC)/sbm_sad_wide.hip $(CSRC)/sbm_sad_fast.hip $(CSRC)/sbm_sad_fast_pw1.hip $(CSRC)/sbm_sad_fast_pw2.hip $(CSRC)/sbm_sad_fast_pw3.hip $(CSRC)/sbm_lrcheck.hip $(CSRC)/sbm_speckle.hip $(CSRC)/sbm_consume.hip $(CSRC)/sbm_rectify.hip $(CSRC)/sbm_fpga.hip $(CSRC)/sbm_gftt.hip $(CSRC)/sbm_gftt_select.hip $(CSRC)/sbm_gftt_cv.hip $(CSRC)/sbm_orb.hip $(CSRC)/sbm_match.hip $(CSRC)/sbm_pnp.hip $(CSRC)/sbm_lk.hip $(CSRC)/sbm_sgbm.hip $(CSRC)/sbm_occupancy.hip $(CSRC)/sbm_occ_rays.hip $(CSRC)/sbm_occ_options.hip $(CSRC)/sbm_occ_grow.hip $(CSRC)/sbm_occ_edit.hip $(CSRC)/sbm_occ_color.hip $(CSRC)/sbm_occ_color_host.hip $(CSRC)/sbm_occ_stamp.hip $(CSRC)/sbm_occ_query.hip $(CSRC)/sbm_occ_tree.hip $(CSRC)/sbm_occ_planner.hip $(CSRC)/sbm_occ_bt.hip $(CSRC)/sbm_occ_load.hip $(CSRC)/sbm_occ_ot.hip $(CSRC)/sbm_occ_ot_host.hip $(CSRC)/sbm_vwd.hip $(CSRC)/sbm_pgo.hip $(CSRC)/sbm_pgo_plan.hip
OBJS := $(SRCS:.hip=.o)

all: $(LIB) oracle

FAST_HDRS := $(CSRC)/sbm_sad_fast_core.h $(CSRC)/sbm_sad_fast_strip.h $(CSRC)/sbm_sad_fast_kernel.h $(CSRC)/sbm_sad_border_wave.h
$(CSRC)/sbm_sad_fast.o $(CSRC)/sbm_sad_fast_pw1.o $(CSRC)/sbm_sad_fast_pw2.o $(CSRC)/sbm_sad_fast_pw3.o: $(FAST_HDRS)

# motion estimation: its double arithmetic must match the host restatement's, so nothing is contracted (the sources say so too)
$(CSRC)/sbm_pnp.o: $(CSRC)/sbm_pnp_math.h
$(CSRC)/sbm_pnp.o: HIPFLAGS += -ffp-contract=off

# keypoint selections: the trim they share; OpenCV's detector is float arithmetic that must match the host restatement's
$(CSRC)/sbm_gftt_select.o $(CSRC)/sbm_gftt_cv.o: $(CSRC)/sbm_gftt_trim.h
$(CSRC)/sbm_gftt_cv.o: HIPFLAGS += -ffp-contract=off

# LK stereo: the tracker's float sums and its double tests must match the host restatement's
$(CSRC)/sbm_lk.o: HIPFLAGS += -ffp-contract=off

# occupancy map: one file per family over sbm_occ.h; the point arithmetic it shares with the other consumers of the map; its
# float and double steps must match the host restatement's
OCC_OBJS := $(CSRC)/sbm_occupancy.o $(CSRC)/sbm_occ_rays.o $(CSRC)/sbm_occ_options.o $(CSRC)/sbm_occ_grow.o $(CSRC)/sbm_occ_edit.o $(CSRC)/sbm_occ_color.o $(CSRC)/sbm_occ_color_host.o $(CSRC)/sbm_occ_stamp.o $(CSRC)/sbm_occ_query.o $(CSRC)/sbm_occ_tree.o $(CSRC)/sbm_occ_planner.o $(CSRC)/sbm_occ_bt.o $(CSRC)/sbm_occ_load.o $(CSRC)/sbm_occ_ot.o $(CSRC)/sbm_occ_ot_host.o
$(OCC_OBJS): $(CSRC)/sbm_occ.h
$(CSRC)/sbm_consume.o $(OCC_OBJS): $(CSRC)/sbm_consume_math.h
$(OCC_OBJS): HIPFLAGS += -ffp-contract=off

# visual-word dictionary: the NNDR test and the likelihood's float steps must match the host restatement's
$(CSRC)/sbm_vwd.o: HIPFLAGS += -ffp-contract=off

# pose-graph optimiser: the kernels and the host-only plan over sbm_pgo.h; its fp64 edge arithmetic and the robust loop's pose
# propagation must match the host restatement's operation for operation
PGO_OBJS := $(CSRC)/sbm_pgo.o $(CSRC)/sbm_pgo_plan.o
$(PGO_OBJS): $(CSRC)/sbm_pgo.h
$(PGO_OBJS): HIPFLAGS += -ffp-contract=off

$(CSRC)/%.o: $(CSRC)/%.hip $(CSRC)/sbm_common.h $(CSRC)/sbm_carve.h $(CSRC)/sbm_handle.h include/sbm.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIB): $(OBJS)
	@mkdir -p $(PKG)/lib
	$(HIPCC) --offload-arch=gfx950 --offload-compress -shared -fPIC -o $@ $(OBJS)

oracle:
	$(MAKE) -C oracle

clean:
	rm -f $(OBJS) $(LIB)
	$(MAKE) -C oracle clean

.PHONY: all oracle clean
