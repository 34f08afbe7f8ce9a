# TEST INFRASTRUCTURE: the emulator library of Makefile plus restarted GMRES (kk_gmres.hip) and the triangular solve its LUPrec calls
# (kk_sptrsv.hip), for tests/test_emu_gmres.py.  Makefile itself stays as it is; its objects are shared.
include Makefile
kk_sptrsv.emu.o: $(CSRC)/kk_levels.h
libkkamd_emu_gmres.so: $(OBJS) kk_gmres.emu.o kk_sptrsv.emu.o
	$(CXX) -shared -o $@ $(OBJS) kk_gmres.emu.o kk_sptrsv.emu.o
