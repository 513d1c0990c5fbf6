// cbet_hd.h -- CBET_HD, the one spelling of "this function is the kernel's and the host's": every header whose statements
// run on both sides (cbet_relocate.h, cbet_node_model.h and the models over it) takes it from here.
#ifndef CBET_HD_H_
#define CBET_HD_H_

#if defined(__HIP__)
#define CBET_HD __attribute__((host)) __attribute__((device)) __attribute__((always_inline)) inline
#else
#define CBET_HD inline
#endif

#endif
