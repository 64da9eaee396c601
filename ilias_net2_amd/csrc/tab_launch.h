/*
 * tab_launch.h -- internal interface between the host unit of the bulk table
 * updates (net2_tabs.cpp) and their kernels (tab_kernels.hip).  Not installed;
 * the public surface is net2_burst_keytab_update / net2_burst_ciphertab_update
 * in include/net2/packet.h.
 */
#ifndef NET2_TAB_LAUNCH_H
#define NET2_TAB_LAUNCH_H

#include "aes_launch.h"
#include "sha2_launch.h"

/*
 * One launch over n records (TabHashRec / TabCipherRec, net2_tab_ops.h; at most
 * one per slot), asynchronous on s and ordered with the bursts there.  d_recs:
 * the device pointer of the page-locked staging that holds them; every lane
 * zeroes the record it read, so the staging holds no key once the kernel has
 * run.  tab / slots: the table's entries.  alg: the key table's HMAC row.
 */
hipError_t net2_launch_keytab_update(int alg, Net2KeyEnt *tab, uint32_t slots,
    void *d_recs, uint32_t n, hipStream_t s);
hipError_t net2_launch_ciphertab_update(Net2CipherEnt *tab, uint32_t slots,
    void *d_recs, uint32_t n, hipStream_t s);

#endif /* NET2_TAB_LAUNCH_H */
