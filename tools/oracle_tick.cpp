// oracle_tick.cpp — TEST INFRASTRUCTURE ONLY (tools/liboracle_tick.so).
//
// The oracle (oracle/aero_oracle.cpp) with one more entry point: AeroL's 1 s
// DCD QTimer slot, callable between two messages of any channel.  The oracle's
// own ORACLE_DCD_TICK runs the timer on the sample clock of a continuous OQPSK
// channel only; a burst channel's timer slot runs from the event loop, that is
// between two writeData calls, so the caller decides where it fires
// (tests/oracle_tick.py: at the end of every message that crosses a multiple
// of Fs samples, what AERO_F_DCD_TICK_BURST does).  Nothing is restated here:
// the oracle is compiled as it stands, and this file adds the hook.
#include "../oracle/aero_oracle.cpp"

extern "C" void oracle_x_dcd_tick(oracle_chan *c) { c->aerol().updateDCD(); }
