# TEST INFRASTRUCTURE: the emulator library of Makefile plus ParILUT (kk_par_ilut.hip), which runs its product and its transposes through
# kk_spgemm.hip and kk_util.hip of the shared objects, for tests/test_emu_par_ilut.py.  Makefile itself stays as it is.
include Makefile
libkkamd_emu_par_ilut.so: $(OBJS) kk_par_ilut.emu.o
	$(CXX) -shared -o $@ $(OBJS) kk_par_ilut.emu.o
