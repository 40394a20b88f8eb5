// zpq_pipe_log.hip -- level 2's dense wave-pipelined encoder keeping the dirty-line log (k_pipe's DLOG form, zpq_dev.h) as a
// kernel of its own name, k_lpipe: zpq_pipe.hip's kernel text compiled once more, for that one instantiation, with its host
// side left out.  zpq_launch_pipe launches it through zpq_launch_lpipe.
#define ZPQ_PIPE_LOG_TU
#include "zpq_pipe.hip"
