# Builds libsim3opt.so (hipcc, gfx950), the CPU oracle and the C++ examples without Python.
#   make                 -> sim3opt_amd/libsim3opt.so, oracle/liboracle_sim3.so
#   make example         -> examples/direct_pgo (testDirectSim3Optimization on the g2o-named shim)
#   make conformance     -> tests/cxx/shim_conformance, tests/cxx/ba_shim_conformance (one block per
#                           method of the g2o-named shims; EIGEN_INC=-I/usr/include/eigen3 for a real Eigen),
#                           tests/cxx/two_view_conformance (the two-view refinement helper),
#                           tests/cxx/pnp_conformance (the PnP RANSAC helper feeding it),
#                           tests/cxx/match_conformance (the matching helper feeding that),
#                           tests/cxx/essential_conformance (the essential-matrix RANSAC helper),
#                           tests/cxx/homography_conformance (the homography MLESAC helper),
#                           tests/cxx/sim3_batch_conformance (the Sim(3) measurement and information helper),
#                           tests/cxx/place_conformance (the place-recognition helper that names the candidates),
#                           tests/cxx/vocabulary_conformance (the trainer of the tree that helper descends),
#                           tests/cxx/surf_conformance (the extractor of the keypoints and descriptors all of them take),
#                           tests/cxx/frames_conformance (the frame store those stages share on the device),
#                           tests/cxx/tracks_conformance (the loop tracks that carry the matches into the bundle adjustment)
#   make LIB=/some/where/libsim3opt.so   builds the library elsewhere (used by the tests)
HIPCC ?= /opt/rocm/bin/hipcc
CSRC  := sim3opt_amd/csrc
# one list of translation units, shared with sim3opt_amd/build.py
SRCS  := $(addprefix $(CSRC)/,$(shell cat $(CSRC)/SOURCES))
HDRS  := $(wildcard $(CSRC)/*.hpp) include/sim3opt.h include/sim3opt_bench.h $(CSRC)/SOURCES
LIB   ?= sim3opt_amd/libsim3opt.so
LIBDIR = $(abspath $(dir $(LIB)))
EIGEN_INC ?= -Itests/mock_eigen

all: $(LIB) oracle/liboracle_sim3.so

$(LIB): $(SRCS) $(HDRS)
	$(HIPCC) --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -Wall -Wno-unused-result -pthread -o $@ $(SRCS) -ldl

oracle/liboracle_sim3.so: oracle/sim3_oracle.c oracle/sim3_oracle.h
	$(MAKE) -C oracle liboracle_sim3.so

example: $(LIB) examples/direct_pgo.cpp include/sim3opt_g2o.hpp
	g++ -std=c++17 -Wall -DSIM3OPT_G2O_NAMES -Iinclude examples/direct_pgo.cpp -L$(LIBDIR) -lsim3opt \
	    -Wl,-rpath,$(LIBDIR) -o examples/direct_pgo

conformance: $(LIB) tests/cxx/shim_conformance.cpp tests/cxx/ba_shim_conformance.cpp tests/cxx/two_view_conformance.cpp \
             tests/cxx/pnp_conformance.cpp include/sim3opt_g2o.hpp include/sim3opt_g2o_ba.hpp include/sim3opt_two_view.hpp \
             include/sim3opt_pnp.hpp tests/cxx/match_conformance.cpp include/sim3opt_match.hpp \
             tests/cxx/essential_conformance.cpp include/sim3opt_essential.hpp \
             tests/cxx/homography_conformance.cpp include/sim3opt_homography.hpp \
             tests/cxx/sim3_batch_conformance.cpp include/sim3opt_sim3_batch.hpp \
             tests/cxx/place_conformance.cpp include/sim3opt_place.hpp \
             tests/cxx/vocabulary_conformance.cpp include/sim3opt_vocabulary.hpp \
             tests/cxx/surf_conformance.cpp include/sim3opt_surf.hpp \
             tests/cxx/frames_conformance.cpp include/sim3opt_frames.hpp \
             tests/cxx/tracks_conformance.cpp include/sim3opt_tracks.hpp
	g++ -std=c++17 -Wall -DSIM3OPT_G2O_NAMES -Iinclude $(EIGEN_INC) tests/cxx/shim_conformance.cpp \
	    -L$(LIBDIR) -lsim3opt -Wl,-rpath,$(LIBDIR) -o tests/cxx/shim_conformance
	g++ -std=c++17 -Wall -DSIM3OPT_G2O_BA_NAMES -Iinclude $(EIGEN_INC) tests/cxx/ba_shim_conformance.cpp \
	    -L$(LIBDIR) -lsim3opt -Wl,-rpath,$(LIBDIR) -o tests/cxx/ba_shim_conformance
	g++ -std=c++17 -Wall -Iinclude tests/cxx/two_view_conformance.cpp \
	    -L$(LIBDIR) -lsim3opt -Wl,-rpath,$(LIBDIR) -o tests/cxx/two_view_conformance
	g++ -std=c++17 -Wall -Iinclude tests/cxx/pnp_conformance.cpp \
	    -L$(LIBDIR) -lsim3opt -Wl,-rpath,$(LIBDIR) -o tests/cxx/pnp_conformance
	g++ -std=c++17 -Wall -Iinclude tests/cxx/match_conformance.cpp \
	    -L$(LIBDIR) -lsim3opt -Wl,-rpath,$(LIBDIR) -o tests/cxx/match_conformance
	g++ -std=c++17 -Wall -Iinclude tests/cxx/essential_conformance.cpp \
	    -L$(LIBDIR) -lsim3opt -Wl,-rpath,$(LIBDIR) -o tests/cxx/essential_conformance
	g++ -std=c++17 -Wall -Iinclude tests/cxx/homography_conformance.cpp \
	    -L$(LIBDIR) -lsim3opt -Wl,-rpath,$(LIBDIR) -o tests/cxx/homography_conformance
	g++ -std=c++17 -Wall -Iinclude tests/cxx/sim3_batch_conformance.cpp \
	    -L$(LIBDIR) -lsim3opt -Wl,-rpath,$(LIBDIR) -o tests/cxx/sim3_batch_conformance
	g++ -std=c++17 -Wall -Iinclude tests/cxx/place_conformance.cpp \
	    -L$(LIBDIR) -lsim3opt -Wl,-rpath,$(LIBDIR) -o tests/cxx/place_conformance
	g++ -std=c++17 -Wall -Iinclude tests/cxx/vocabulary_conformance.cpp \
	    -L$(LIBDIR) -lsim3opt -Wl,-rpath,$(LIBDIR) -o tests/cxx/vocabulary_conformance
	g++ -std=c++17 -Wall -Iinclude tests/cxx/surf_conformance.cpp \
	    -L$(LIBDIR) -lsim3opt -Wl,-rpath,$(LIBDIR) -o tests/cxx/surf_conformance
	g++ -std=c++17 -Wall -Iinclude tests/cxx/frames_conformance.cpp \
	    -L$(LIBDIR) -lsim3opt -Wl,-rpath,$(LIBDIR) -o tests/cxx/frames_conformance
	g++ -std=c++17 -Wall -Iinclude tests/cxx/tracks_conformance.cpp \
	    -L$(LIBDIR) -lsim3opt -Wl,-rpath,$(LIBDIR) -o tests/cxx/tracks_conformance

clean:
	rm -f sim3opt_amd/libsim3opt.so oracle/liboracle_sim3.so examples/direct_pgo tests/cxx/shim_conformance \
	    tests/cxx/ba_shim_conformance tests/cxx/two_view_conformance tests/cxx/pnp_conformance tests/cxx/match_conformance \
	    tests/cxx/essential_conformance tests/cxx/homography_conformance tests/cxx/sim3_batch_conformance \
	    tests/cxx/place_conformance tests/cxx/vocabulary_conformance tests/cxx/surf_conformance \
	    tests/cxx/frames_conformance tests/cxx/tracks_conformance

.PHONY: all example conformance clean
