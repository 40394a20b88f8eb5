// zpq_chain_log.hip -- level 2's dense two-hypothesis decoder keeping the dirty-line log (k_chain's DLOG form, zpq_dev.h)
// as a kernel of its own name, k_lchain: zpq_chain.hip's kernel text compiled once more, for that one instantiation, with
// its host side left out.  zpq_launch_chain launches it through zpq_launch_lchain.
#define ZPQ_CHAIN_LOG_TU
#include "zpq_chain.hip"
