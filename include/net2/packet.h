/*
 * net2/packet.h -- the SHA-2 uses of the packet codec (types/packet.n2t)
 * on the MI355X path: IV derivation from a packet header
 * (net2_ph_to_iv, packet.n2t:100-158), and the hash steps of
 * net2_packet_encode / net2_packet_decode (packet.n2t:341-463 / :170-336)
 * for whole bursts of datagrams under one connection's keys or, with a
 * device key table, under the keys of each datagram's own connection.
 */
#ifndef NET2_PACKET_H
#define NET2_PACKET_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* struct packet_header of packet.n2t:89-95; encoded as two big-endian
 * uint32 (net2_ph_overhead = 8, packet.n2t:97). */
struct net2_packet_header {
	uint32_t	seq;
	uint32_t	flags;
};

/*
 * net2_ph_to_iv_buf: the reference's net2_ph_to_iv (a decoded header in,
 * the IV into a plain buffer; the reference's own name and prototype stay
 * the reference's, packet.n2t:100-158).  iv = first ivlen bytes of the chain
 * iv += SHA-256(ph_network || iv) (packet.n2t:127-144), any ivlen.
 * Synchronous, one header; the SHA-256s run on the GPU.
 * 0, EINVAL, ENOMEM, ENODEV or EIO.
 */
int net2_ph_to_iv_buf(const struct net2_packet_header *ph, size_t ivlen,
    void *iv);

/*
 * Batched form for a whole datagram batch, device-resident: header i is
 * (d_seq[i], d_flags[i]), its IV goes to d_iv + i * ivlen.  ivlen <= 64
 * (two SHA-256 rounds; AES-256-CBC, the reference's only cipher, needs 16,
 * src/enc.c:72-73).  Asynchronous on stream.
 */
int net2_ph_to_iv_dev(const uint32_t *d_seq, const uint32_t *d_flags,
    uint64_t n, uint32_t ivlen, void *d_iv, void *stream);

/* Packet header flags used here (types/packet.n2t:27-28) and the result
 * codes of net2_packet_decode / _encode (:44-47, :53-56). */
#define NET2_PH_ENCRYPTED	0x00000001
#define NET2_PH_SIGNED		0x00000002
#define NET2_PDECODE_OK		0
#define NET2_PDECODE_RESOURCE	1
#define NET2_PDECODE_BAD	2
#define NET2_PDECODE_UNSAFE	3
#define NET2_PENCODE_OK		0
#define NET2_PENCODE_RESOURCE	1
#define NET2_PENCODE_BAD	2
#define NET2_PENCODE_UNSAFE	3

/*
 * Device scratch (bytes, 16-byte aligned) of a burst of n datagrams.  Its
 * length-binning area comes first, at the same place for every n: one
 * workspace serves bursts of any size up to its own, and
 * net2_sha2_workspace_init / net2_sha2_workspace_stats (net2/sha2_batch.h)
 * prepare and inspect it.  A keyed burst of at most 16 datagrams per SIMD
 * of the device (16,384 on an MI355X) is hashed 1 to 16 datagrams per
 * workgroup, in one launch, without touching the workspace; a larger one
 * below 65,536 datagrams (at most one wave per SIMD) is hashed in arrival
 * order, without the binning launch (net2_sha2_burst_limits below).
 */
size_t net2_packet_burst_workspace(uint64_t n);

/*
 * Size thresholds of the keyed bursts, process-wide (diagnostics, tests and
 * A/B runs): wave_max is the largest burst hashed by the one-launch
 * small-burst form (0: never), bin_min the smallest burst whose datagrams
 * are length-binned first.  A value < 0 restores that threshold's default
 * (16 datagrams per SIMD / 65,536, or NET2_BURST_WAVE_MAX /
 * NET2_BURST_BIN_MIN when set in the environment at first use).  Results do
 * not depend on either; only the time does.  Both apply to the
 * single-connection calls, their _host pipelines and the _mc calls below
 * alike.  Always 0.
 */
int net2_sha2_burst_limits(int64_t wave_max, int64_t bin_min);

/*
 * Keyed hash-burst launches of this process so far, by form (either pointer
 * may be NULL): lane_launches counts the one-datagram-per-lane kernel,
 * wave_launches the one-launch small-burst form -- one per keyed pass through
 * net2_packet_{decode,encode}_burst[_ck], per chunk of their _host pipelines,
 * and per net2_packet_{decode,encode}_burst_mc call.  Bursts without a hash
 * key, calls with n == 0 and calls refused by their argument checks count
 * nothing.  The only way to tell which form a call took.  Host state: needs
 * no device.  Always 0.
 */
int net2_sha2_burst_stats(uint64_t *lane_launches, uint64_t *wave_launches);

/*
 * RX: the hash steps of net2_packet_decode for a burst of n received
 * datagrams under one connection's rx keys, device-resident and
 * asynchronous on `stream` (one stream, no host synchronisation).
 * Datagram i = d_base[d_offsets[i] .. + d_lens[i]) as it came off the wire:
 * 8-byte header (seq, flags big-endian), then the HMAC field when
 * PH_SIGNED, then the payload.  hash_alg is the negotiated keyed hash
 * (HMAC row 4..6, key of its registry length) or 0 for none; enc_alg != 0
 * when an encryption key is negotiated, ivlen its IV length (<= 64;
 * AES-256-CBC: 16, src/enc.c:72-73).  Per datagram, as packet.n2t does:
 *   - shorter than the header: NET2_PDECODE_BAD (:196-198);
 *   - PH_SIGNED / PH_ENCRYPTED missing while the key is set:
 *     NET2_PDECODE_UNSAFE (:215-221);
 *   - PH_SIGNED: the hash field is compared with HMAC(key, rest); too
 *     short or unequal: NET2_PDECODE_BAD (:226-258);
 *   - PH_ENCRYPTED and OK: the IV for the decryption step,
 *     net2_ph_to_iv (:263-279), to d_iv + i * ivlen (d_iv may be NULL).
 * d_result[i] receives the code; d_seq / d_flags (both or neither) the
 * decoded header.  The decryption itself (:283-292) is
 * net2_packet_decrypt_burst below; the window check and the key commit
 * (:200-206, :293-313) stay with the caller.
 */
int net2_packet_decode_burst(int hash_alg, const void *hash_key,
    size_t hash_keylen, int enc_alg, uint32_t ivlen, const void *d_base,
    const uint64_t *d_offsets, const uint32_t *d_lens, uint64_t n,
    uint8_t *d_result, void *d_iv, uint32_t *d_seq, uint32_t *d_flags,
    void *d_ws, size_t ws_bytes, void *stream);

/*
 * RX under a connection's full rx key state (src/conn_keys.c): during a key
 * rollover a datagram may be sealed with the alternate key.  As
 * net2_ck_rx_key (src/conn_keys.c:447-476) decides for every datagram after
 * its header is decoded (packet.n2t:210), the kernel verifies datagram i
 * with the alternate key when alt_hash_key != NULL (an alternate key is
 * installed, NET2_CK_RX_ALT) and either its flags carry PH_ALTKEY or, unless
 * alt_no_cutoff (NET2_CK_F_NO_RX_CUTOFF), seq - rx_start >=
 * alt_cutoff - rx_start (rx_start: the window's cw_rx_start); otherwise with
 * the active key.  The alternate key is new key material under the same
 * negotiated algorithms (hash_alg, enc_alg; alt_hash_keylen must equal
 * hash_keylen).  Everything else as net2_packet_decode_burst, which is this
 * call with alt_hash_key == NULL.  Committing the alternate key
 * (net2_ck_rx_key_commit, :487-510) stays with the caller.
 */
#define NET2_PH_ALTKEY		0x80000000	/* types/packet.n2t:34 */
struct net2_burst_rx_keys {
	int hash_alg;		/* 0 or an HMAC row (4..6) */
	const void *hash_key;	/* the active key */
	size_t hash_keylen;
	int enc_alg;		/* != 0: a cipher key is set */
	const void *alt_hash_key;	/* NULL: no alternate key */
	size_t alt_hash_keylen;
	int alt_no_cutoff;
	uint32_t alt_cutoff;
	uint32_t rx_start;
};
int net2_packet_decode_burst_ck(const struct net2_burst_rx_keys *keys,
    uint32_t ivlen, const void *d_base, const uint64_t *d_offsets,
    const uint32_t *d_lens, uint64_t n, uint8_t *d_result, void *d_iv,
    uint32_t *d_seq, uint32_t *d_flags, void *d_ws, size_t ws_bytes,
    void *stream);

/*
 * TX: the hash steps of net2_packet_encode for a burst.  Datagram slot i =
 * d_base[d_offsets[i] .. + d_lens[i]) holds, on entry, 8 bytes for the
 * header, then hashlen reserved bytes when d_flags[i] has PH_SIGNED (as
 * connection.c:336-339 reserves them), then the payload -- already
 * encrypted when PH_ENCRYPTED (its IV comes from net2_ph_to_iv_dev first,
 * the encryption from net2_packet_encrypt_burst below).
 * The flags are checked against the keys both ways (NET2_PENCODE_UNSAFE,
 * :364-370); then the header (d_seq[i], d_flags[i]) is written big-endian
 * and, when PH_SIGNED, the HMAC of the payload into the reserved field
 * (:410-443).  The transmitter picks the key before it builds a datagram
 * (net2_ck_tx_key, src/conn_keys.c:544-580, sets PH_ALTKEY), so a burst
 * under the alternate tx key is a call with that key.  A slot too short for header and field gets
 * NET2_PENCODE_RESOURCE and is left untouched.  Codes to d_result.
 */
int net2_packet_encode_burst(int hash_alg, const void *hash_key,
    size_t hash_keylen, int enc_alg, const uint32_t *d_seq,
    const uint32_t *d_flags, void *d_base, const uint64_t *d_offsets,
    const uint32_t *d_lens, uint64_t n, uint8_t *d_result, void *d_ws,
    size_t ws_bytes, void *stream);

/*
 * The payload cipher of a burst: the decryption step of net2_packet_decode
 * (packet.n2t:263-292) after net2_packet_decode_burst{,_ck}, and the
 * encryption step of net2_packet_encode (:375-398) before
 * net2_packet_encode_burst, each on the same stream as its hash burst,
 * device-resident and asynchronous (no host synchronisation).  The cipher is
 * the reference's one real cipher, aes256 (src/enc.c:70-74): AES-256-CBC as
 * OpenSSL's EVP runs it, PKCS#7 padding included (:316-413), bit for bit.
 *
 * The payload of datagram i starts po(i) = 8 + (flags[i] & PH_SIGNED ?
 * hashlen : 0) bytes into the datagram, at any alignment; its IV is the 16
 * bytes at d_iv + 16 * i, as the decode burst and net2_ph_to_iv_dev write
 * them with ivlen 16.  The round keys are expanded on the host inside the
 * call and travel in the launch's arguments, so the keys need not outlive it.
 *
 * Both return 0, EINVAL (enc_alg not NET2_ENC_AES256, a key or alternate key
 * that is not 32 bytes, hashlen not 0, 32, 48 or 64, a NULL pointer while
 * n > 0, or the alternate-key mismatches below -- all checked before the
 * device), ENOMEM, ENODEV or EIO; n == 0 is 0 and launches nothing.
 */
#define NET2_ENC_NIL		0
#define NET2_ENC_AES256		1	/* src/enc.c:70-74 */
struct net2_burst_cipher_keys {
	int enc_alg;			/* NET2_ENC_AES256 */
	const void *enc_key;		/* the active key, 32 bytes */
	size_t enc_keylen;
	const void *alt_enc_key;	/* NULL: no alternate key */
	size_t alt_enc_keylen;		/* 0 or 32 */
};

/*
 * RX.  keys: the rx key state the hash burst ran under (hashlen is the digest
 * length of keys->hash_alg, 0 without one); d_seq, d_flags, d_iv, d_result:
 * that burst's outputs.  Only a datagram with d_result[i] == NET2_PDECODE_OK
 * and PH_ENCRYPTED is decrypted; every other one keeps its code, gets
 * d_plen[i] = 0, and nothing of it is written.  A key set carries both keys:
 * datagram i takes ck->alt_enc_key exactly where the hash step took the
 * alternate hash key (net2_ck_rx_key, src/conn_keys.c:447-476, over
 * keys->alt_*, rx_start, d_seq[i], d_flags[i]); an alternate key is installed
 * when keys->alt_hash_key != NULL, and then ck->alt_enc_key must be set, d_seq
 * must be given and keys->hash_alg must not be 0 (EINVAL otherwise).
 * The ciphertext is the d_lens[i] - po(i) bytes of the payload.  Empty, not a
 * multiple of 16, or with a last block that fails EVP's padding check (the
 * last byte v in 1..16, the last v bytes all v): d_result[i] =
 * NET2_PDECODE_BAD, d_plen[i] = 0 (net2_encctx_encbuf returning NULL,
 * :288-291), and nothing of the datagram is written.  Otherwise the plaintext
 * goes to d_out + d_offsets[i] + po(i) and its length to d_plen[i]; what
 * follows it within the datagram's own bytes of d_out is unspecified.  No
 * byte outside a decrypted datagram's payload is written.  d_out == d_base
 * decrypts in place; any other d_out must not overlap the burst.
 */
int net2_packet_decrypt_burst(const struct net2_burst_rx_keys *keys,
    const struct net2_burst_cipher_keys *ck, const void *d_base,
    const uint64_t *d_offsets, const uint32_t *d_lens, uint64_t n,
    const uint32_t *d_seq, const uint32_t *d_flags, const void *d_iv,
    uint8_t *d_result, void *d_out, uint32_t *d_plen, void *stream);

/*
 * TX.  Slot i holds d_plen[i] plaintext bytes at po(i).  Without
 * PH_ENCRYPTED it is left as it is: d_wire_len[i] = po + plen, the code
 * NET2_PENCODE_OK, or NET2_PENCODE_RESOURCE when that exceeds d_lens[i].
 * With PH_ENCRYPTED the payload becomes clen = 16 * (plen / 16 + 1) bytes
 * (EVP always pads: an empty plaintext is one block): when po + clen >
 * d_lens[i] the code is NET2_PENCODE_RESOURCE, the slot untouched and
 * d_wire_len[i] = 0; otherwise it is encrypted in place and d_wire_len[i] =
 * po + clen.  d_wire_len is what net2_packet_encode_burst takes as d_lens;
 * the checks of the flags against the keys stay there.  ck's alternate key is
 * not used (the transmitter picks the key set before it builds a datagram).
 */
int net2_packet_encrypt_burst(const struct net2_burst_cipher_keys *ck,
    uint32_t hashlen, const uint32_t *d_flags, const void *d_iv,
    void *d_base, const uint64_t *d_offsets, const uint32_t *d_lens,
    const uint32_t *d_plen, uint64_t n, uint8_t *d_result,
    uint32_t *d_wire_len, void *stream);

/*
 * Size threshold of the decrypt bursts, process-wide (diagnostics, tests and
 * A/B runs), for net2_packet_decrypt_burst and net2_packet_decrypt_burst_mc
 * alike: wave_max is the largest burst decrypted one wave per datagram, the
 * datagram's blocks spread over the wave's lanes (0: never); a larger burst
 * is decrypted one lane per datagram.  A value < 0 restores the default (the
 * measured crossover, 65,536 datagrams on an MI355X, or NET2_AES_WAVE_MAX
 * when set in the environment at first use).  Results do not depend on it --
 * codes, lengths and every output byte are the same in both forms -- only the
 * time does.  The encrypt bursts have a threshold of their own
 * (net2_aes_encrypt_limits).  Always 0; needs no device.
 */
int net2_aes_burst_limits(int64_t wave_max);

/*
 * Decrypt launches of this process so far, by form (either pointer may be
 * NULL): the only way to tell which form a call took.  A call with n == 0
 * or one refused by its argument checks launches nothing.  Always 0.
 */
int net2_aes_burst_stats(uint64_t *lane_launches, uint64_t *wave_launches);

/*
 * Size threshold of the encrypt bursts, process-wide (diagnostics, tests and
 * A/B runs), for net2_packet_encrypt_burst and net2_packet_encrypt_burst_mc
 * alike: quad_max is the largest burst encrypted four lanes per datagram, one
 * column of the AES state each (0: never); a larger burst is encrypted one
 * lane per datagram.  A value < 0 restores the default (the measured
 * crossover on an MI355X, DESIGN.md 5.5.7, or NET2_AES_QUAD_MAX when set in
 * the environment at first use).  Results do not depend on it -- codes,
 * d_wire_len and every output byte are the same in both forms -- only the
 * time does.  Always 0; needs no device.
 */
int net2_aes_encrypt_limits(int64_t quad_max);

/*
 * Encrypt launches of this process so far, by form (either pointer may be
 * NULL): the only way to tell which form a call took.  A call with n == 0
 * or one refused by its argument checks launches nothing.  Always 0.
 */
int net2_aes_encrypt_stats(uint64_t *lane_launches, uint64_t *quad_launches);

/*
 * Keyed bursts over many connections.  The reference terminates many
 * connections on one UDP socket (src/udp_connection.c:81-170: net2_conn_p2p
 * keyed by remote address under one net2_udpsocket), so what a receive loop
 * takes off the socket is the datagrams of many connections interleaved,
 * each connection with its own negotiated key and rollover state.  A
 * net2_burst_keytab holds that state on the device, one entry ("slot") per
 * connection; the _mc calls below take the table and, per datagram, the slot
 * of its connection, and hash every datagram under its own keys in one call.
 *
 * A table lives in the memory of the device that is current when it is
 * created and serves one keyed hash (HMAC row 4..6); connections that
 * negotiated another row go to another table, connections without a hash
 * key need none (net2_packet_decode_burst with hash_alg 0).  Every slot
 * starts with neither side set.
 *
 *   net2_burst_keytab_set_rx  the slot's rx side from a connection's rx key
 *       state (keys->hash_alg must be the table's row; the alternate key,
 *       cutoff, rx_start and enc_alg as for net2_packet_decode_burst_ck);
 *   net2_burst_keytab_set_tx  its tx side: the key the transmitter seals
 *       with (net2_ck_tx_key) and whether a cipher key is set;
 *   net2_burst_keytab_clear   both sides unset (the connection is gone).
 *
 * Each is asynchronous on `stream` and ordered with the bursts there: a
 * burst enqueued on the same stream before the call sees the old entry, one
 * enqueued after it the new one -- a key commit (net2_ck_rx_key_commit,
 * src/conn_keys.c:487-510) lands between two bursts without a host
 * synchronisation.  The keys are consumed before the call returns (the entry
 * travels in the launch's arguments), so they need not outlive it, and a
 * slot set twice in a row ends with the second.  Work on other streams is
 * not ordered with an update; the caller orders it as for any device memory.
 * net2_burst_keytab_destroy waits for the device and frees the table.
 *
 * 0, EINVAL (a row that is not 4..6, keys->hash_alg not the table's, a key or
 * alternate key of another length than the row's, slot >= slots, slots == 0,
 * a NULL argument, or -- checked last -- a calling thread whose current
 * device is not the table's), ENOMEM, ENODEV or EIO.
 */
struct net2_burst_keytab;
int net2_burst_keytab_create(int hash_alg, uint32_t slots,
    struct net2_burst_keytab **tab);
void net2_burst_keytab_destroy(struct net2_burst_keytab *tab);
int net2_burst_keytab_set_rx(struct net2_burst_keytab *tab, uint32_t slot,
    const struct net2_burst_rx_keys *keys, void *stream);
int net2_burst_keytab_set_tx(struct net2_burst_keytab *tab, uint32_t slot,
    const void *key, size_t keylen, int enc_alg, void *stream);
int net2_burst_keytab_clear(struct net2_burst_keytab *tab, uint32_t slot,
    void *stream);

/*
 * The result code of a datagram without a connection in the _mc calls:
 * d_conn[i] >= slots, or the slot's rx (decode) / tx (encode) side is not
 * set.  (4 is the reference's NET2_PDECODE_WINDOW, which stays the
 * caller's.)
 */
#define NET2_PBURST_NOCONN	5

/*
 * net2_packet_decode_burst_ck / net2_packet_encode_burst with the keys of
 * datagram i taken from slot d_conn[i] of `tab` (d_conn: n uint32 in device
 * memory).  Everything else as in those calls: the same workspace
 * (net2_packet_burst_workspace(n)), the same outputs, asynchronous on one
 * stream; ivlen is one per call (the reference has one cipher), and an IV
 * is due only where the datagram's connection has a cipher key.  For
 * identical keys the results are those of the single-connection calls, bit
 * for bit.
 *   RX: a datagram shorter than the header is NET2_PDECODE_BAD whatever its
 *   connection (packet.n2t:196-198 precede the key lookup at :210);
 *   otherwise its header is decoded (d_seq / d_flags), and without a
 *   connection it is NET2_PBURST_NOCONN: nothing hashed, no IV written.
 *   TX: a slot without a connection is NET2_PBURST_NOCONN and left untouched.
 * Both forms of the single-connection calls exist here: a burst of at most
 * net2_sha2_burst_limits' wave_max datagrams (default: 16 per SIMD of the
 * device) is hashed 1 to 16 datagrams per workgroup in one launch, the keys
 * read from the table by every workgroup, and does not touch the workspace
 * (which is required and checked all the same); a larger one is hashed one
 * datagram per lane, and bin_min applies.  Results do not depend on the
 * form; net2_sha2_burst_stats tells which one a call took.  The host form
 * is net2_packet_{decode,encode}_burst_mc_host below.
 * EINVAL also when the calling thread's device is not the table's.
 */
int net2_packet_decode_burst_mc(const struct net2_burst_keytab *tab,
    const uint32_t *d_conn, uint32_t ivlen, const void *d_base,
    const uint64_t *d_offsets, const uint32_t *d_lens, uint64_t n,
    uint8_t *d_result, void *d_iv, uint32_t *d_seq, uint32_t *d_flags,
    void *d_ws, size_t ws_bytes, void *stream);
int net2_packet_encode_burst_mc(const struct net2_burst_keytab *tab,
    const uint32_t *d_conn, const uint32_t *d_seq, const uint32_t *d_flags,
    void *d_base, const uint64_t *d_offsets, const uint32_t *d_lens,
    uint64_t n, uint8_t *d_result, void *d_ws, size_t ws_bytes, void *stream);

/*
 * The payload cipher over many connections.  A net2_burst_ciphertab is to
 * net2_packet_{decrypt,encrypt}_burst what a net2_burst_keytab is to the hash
 * bursts: the cipher keys of many connections on the device, one slot per
 * connection, so the encrypted datagrams of a shared socket's receive batch
 * are decrypted in one call after net2_packet_decode_burst_mc authenticated
 * them in one.  It is a table of its own (the cipher does not depend on the
 * HMAC row; both tables are indexed by the same d_conn).  It lives in the
 * memory of the device that is current when it is created, serves
 * NET2_ENC_AES256, and every slot starts with neither side set.
 *
 *   net2_burst_ciphertab_set_rx  the slot's rx side from exactly the pair
 *       net2_packet_decrypt_burst takes, under the same checks: ck->enc_key,
 *       and ck->alt_enc_key when keys->alt_hash_key != NULL (an alternate key
 *       is installed; then keys->hash_alg must not be 0).  Of `keys` only the
 *       alternate-key state is stored: installed, alt_no_cutoff, alt_cutoff,
 *       rx_start;
 *   net2_burst_ciphertab_set_tx  its tx side: ck->enc_key, the key the
 *       transmitter encrypts with (ck's alternate key is not used);
 *   net2_burst_ciphertab_clear   both sides unset, the slot's keys zeroed.
 *
 * The round keys are expanded on the host inside the call and the new entry
 * travels in the launch's arguments.  So, as for the key table: each call is
 * asynchronous on `stream` and ordered with the bursts there, the keys need
 * not outlive it, a slot set twice in a row ends with the second, and setting
 * one side leaves the other as it is.  Work on other streams is not ordered
 * with an update.  net2_burst_ciphertab_destroy waits for the table's device,
 * zeroes the table there and frees it.
 *
 * 0, EINVAL (enc_alg not NET2_ENC_AES256, slots == 0, slot >= slots, a NULL
 * argument, a key or alternate key that is not 32 bytes, keys->hash_alg
 * neither 0 nor an HMAC row, the alternate-key mismatches of
 * net2_packet_decrypt_burst, or -- checked last -- a calling thread whose
 * current device is not the table's), ENOMEM, ENODEV or EIO.
 */
struct net2_burst_ciphertab;
int net2_burst_ciphertab_create(int enc_alg, uint32_t slots,
    struct net2_burst_ciphertab **tab);
void net2_burst_ciphertab_destroy(struct net2_burst_ciphertab *tab);
int net2_burst_ciphertab_set_rx(struct net2_burst_ciphertab *tab, uint32_t slot,
    const struct net2_burst_rx_keys *keys,
    const struct net2_burst_cipher_keys *ck, void *stream);
int net2_burst_ciphertab_set_tx(struct net2_burst_ciphertab *tab, uint32_t slot,
    const struct net2_burst_cipher_keys *ck, void *stream);
int net2_burst_ciphertab_clear(struct net2_burst_ciphertab *tab, uint32_t slot,
    void *stream);

/*
 * net2_packet_decrypt_burst / net2_packet_encrypt_burst with the keys of
 * datagram i taken from slot d_conn[i] of `tab` (d_conn: n uint32 in device
 * memory).  hashlen is one per call -- 0, 32, 48 or 64: a key table serves one
 * HMAC row, so a _mc hash burst has one digest length.  d_seq is required on
 * RX (any slot may have an alternate key).  Everything not stated here is the
 * contract of the single-connection call, and for identical keys the outputs
 * are those of the single-connection calls, bit for bit.
 *   RX: a datagram whose incoming code is not NET2_PDECODE_OK keeps it
 *   (NET2_PBURST_NOCONN from the hash step included), as does one without
 *   PH_ENCRYPTED: d_plen[i] = 0, nothing written, no table look-up.  An OK
 *   PH_ENCRYPTED datagram with d_conn[i] >= slots, or whose slot's rx side is
 *   not set, becomes NET2_PBURST_NOCONN: d_plen[i] = 0, nothing written (the
 *   reference would run its nil cipher there; the code tells the caller
 *   which datagrams those are).  Otherwise it is decrypted under the slot's
 *   active or alternate key, by net2_ck_rx_key's rule over the slot's own
 *   state, d_seq[i] and d_flags[i] -- the choice the hash step made.
 *   TX: a slot without PH_ENCRYPTED is treated as in the single call (no key,
 *   no look-up).  The room check comes first: NET2_PENCODE_RESOURCE as there.
 *   A PH_ENCRYPTED slot with room whose connection has no tx side is
 *   NET2_PBURST_NOCONN, left untouched, d_wire_len[i] = 0.
 * 0, EINVAL (tab NULL, hashlen not 0, 32, 48 or 64, a NULL pointer while
 * n > 0 -- all before the device check -- or a calling thread whose device
 * is not the table's), ENOMEM, ENODEV or EIO; n == 0 is 0 and launches
 * nothing.
 */
int net2_packet_decrypt_burst_mc(const struct net2_burst_ciphertab *tab,
    const uint32_t *d_conn, uint32_t hashlen, const void *d_base,
    const uint64_t *d_offsets, const uint32_t *d_lens, uint64_t n,
    const uint32_t *d_seq, const uint32_t *d_flags, const void *d_iv,
    uint8_t *d_result, void *d_out, uint32_t *d_plen, void *stream);
int net2_packet_encrypt_burst_mc(const struct net2_burst_ciphertab *tab,
    const uint32_t *d_conn, uint32_t hashlen, const uint32_t *d_flags,
    const void *d_iv, void *d_base, const uint64_t *d_offsets,
    const uint32_t *d_lens, const uint32_t *d_plen, uint64_t n,
    uint8_t *d_result, uint32_t *d_wire_len, void *stream);

/*
 * Bulk updates of the two tables: many slots in one call, the keys prepared
 * on the device.  The per-slot calls above are right for one key commit
 * between two bursts -- one launch each, the entry made on the host.  A
 * server that loads its tables at start-up, or whose connections roll their
 * keys over together, hands the whole list to one call here: the raw keys are
 * staged, and one launch per at most ops_per_launch ops (default 65,536) has a
 * lane per slot compute that slot's HMAC midstates or AES-256 schedules and
 * store its entry.
 *
 * An op is one per-slot call: `op` NET2_BURST_TAB_RX takes exactly what
 * _set_rx takes (key table: `rx`; cipher table: `rx` and `ck`),
 * NET2_BURST_TAB_TX exactly what _set_tx takes (key table: tx_key, tx_keylen,
 * tx_enc_alg; cipher table: `ck`), NET2_BURST_TAB_CLEAR is _clear; fields of
 * the other ops are not looked at.
 *
 * Result: every entry of the table ends byte for byte as if the n per-slot
 * calls had been issued in array order on `stream`.  Several ops on one slot
 * apply in order, RX and TX of one slot both stay, a CLEAR undoes what came
 * before it in the list and not what comes after.
 * Ordering: asynchronous on `stream` and ordered with the bursts there, as
 * the per-slot calls are -- a burst enqueued before the call sees the old
 * entries, one enqueued after it the new ones; a host burst
 * (net2_packet_*_burst_mc_host) sees an update queued on its table_stream
 * before it.  Work on other streams is not ordered with it.
 * Key lifetime: the keys are consumed before the call returns -- `ops` and
 * everything they point to may be overwritten at once.  The library stages
 * them in page-locked memory it owns (per table: a ring of areas, each
 * reused once the launch that read it is done; a call waits on the host only
 * while every area is in flight).  No raw key stays there once the update
 * kernel has run -- each lane zeroes the record it read -- and the staging is
 * wiped again and freed by _destroy.
 * Capture: a `stream` that is being captured (hipStreamIsCapturing) is
 * refused with EINVAL, since a graph cannot own the library's staging; the
 * per-slot calls, whose entry travels in the launch's arguments, stay the
 * form to capture.
 *
 * Every op is checked before any device work, in array order, each by the
 * checks of its per-slot call: on the first bad one the call returns EINVAL,
 * nothing is enqueued, no table byte and no counter changes.  EINVAL also for
 * tab NULL, ops NULL with n > 0, an unknown `op`, n > UINT32_MAX, a capturing
 * stream, and -- checked last -- a calling thread whose current device is not
 * the table's; ENOMEM, ENODEV or EIO otherwise.  n == 0 is 0 and launches
 * nothing.
 */
#define NET2_BURST_TAB_CLEAR 0u
#define NET2_BURST_TAB_RX    1u
#define NET2_BURST_TAB_TX    2u

struct net2_burst_keytab_op {
	uint32_t slot;
	uint32_t op;                    /* NET2_BURST_TAB_{CLEAR,RX,TX} */
	struct net2_burst_rx_keys rx;   /* RX: exactly net2_burst_keytab_set_rx's keys */
	const void *tx_key;             /* TX: exactly net2_burst_keytab_set_tx's */
	size_t tx_keylen;
	int tx_enc_alg;
};
int net2_burst_keytab_update(struct net2_burst_keytab *tab,
    const struct net2_burst_keytab_op *ops, size_t n, void *stream);

struct net2_burst_ciphertab_op {
	uint32_t slot;
	uint32_t op;
	struct net2_burst_rx_keys rx;        /* RX: set_rx's `keys` (the alternate-key state) */
	struct net2_burst_cipher_keys ck;    /* RX: set_rx's `ck`; TX: set_tx's `ck` */
};
int net2_burst_ciphertab_update(struct net2_burst_ciphertab *tab,
    const struct net2_burst_ciphertab_op *ops, size_t n, void *stream);

/*
 * The most ops one launch of a bulk update takes, process-wide (a test knob,
 * like net2_aes_burst_limits): a longer list is cut into launches that keep
 * their order.  A value < 0 restores the default, 65,536; 0 counts as 1.
 * Results do not depend on it.  Always 0; needs no device.
 */
int net2_burst_tab_limits(int64_t ops_per_launch);

/*
 * Table-update launches of this process so far (either pointer may be NULL):
 * those of the per-slot calls of both tables, and those of the bulk updates.
 * A call refused by its argument checks launches nothing.  Host state, needs
 * no device.  Always 0.
 */
int net2_burst_tab_stats(uint64_t *slot_launches, uint64_t *bulk_launches);

/*
 * Fingerprints of table entries: the SHA-256 of each of the n entries from
 * slot `first`, 32 bytes per slot, to d_digests (device memory), asynchronous
 * on `stream` and ordered with the updates there.  Two tables that hold the
 * same keys and state have the same fingerprints, so an operator compares
 * replicas -- and a test a bulk-filled table with a per-slot-filled one --
 * without key material leaving the device.  (A slot's fingerprint covers the
 * whole entry, also the bytes a key-table CLEAR leaves behind.)
 * 0, EINVAL (tab NULL, first + n > slots, d_digests NULL with n > 0, or --
 * checked last -- a calling thread whose device is not the table's), ENODEV
 * or EIO; n == 0 is 0.
 */
int net2_burst_keytab_fingerprint(const struct net2_burst_keytab *tab,
    uint32_t first, uint32_t n, void *d_digests, void *stream);
int net2_burst_ciphertab_fingerprint(const struct net2_burst_ciphertab *tab,
    uint32_t first, uint32_t n, void *d_digests, void *stream);

/*
 * Host-memory bursts: the same hash steps for datagrams that live in host
 * memory -- the reference's case: each received one is a net2_buffer filled
 * by net2_sockdgram_recv (src/sockdgram.c:67-108) and decoded at
 * src/connection.c:199; each sent one is built by gather()
 * (src/connection.c:336-339, :467).  Synchronous; every pointer is host
 * memory (page-locked or pageable, any mix).  The datagrams are packed into
 * pinned staging in 64 MiB chunks (two per device in flight: pack, H2D,
 * kernels, results), sharded over every usable GPU (max_devices <= 0: all;
 * no slice under 16 MiB; the list starts at the calling thread's current
 * device, as net2_sha2_batch), each slice's thread on its GPU's NUMA node.
 * The kernels store results straight into page-locked result arrays and
 * through pinned staging into pageable ones.
 *
 * RX: datagram i = base[offsets[i] .. + lens[i]); result[i] its
 * NET2_PDECODE_* code, iv + i * ivlen its IV when OK and encrypted (iv may
 * be NULL), seq[i] / flags[i] the decoded header (both or neither) --
 * exactly net2_packet_decode_burst_ck's outputs.
 *
 * TX: slot i as for net2_packet_encode_burst, in the caller's buffer: for
 * every slot whose code is NET2_PENCODE_OK the header and (PH_SIGNED) the
 * HMAC field are written into it; the payload bytes are only read.
 *
 * 0, EINVAL, ENOMEM, ENODEV or EIO (then some results may be unset).
 */
int net2_packet_decode_burst_host(const struct net2_burst_rx_keys *keys,
    uint32_t ivlen, const void *base, const uint64_t *offsets,
    const uint32_t *lens, uint64_t n, uint8_t *result, void *iv,
    uint32_t *seq, uint32_t *flags, int max_devices);
int net2_packet_encode_burst_host(int hash_alg, const void *hash_key,
    size_t hash_keylen, int enc_alg, const uint32_t *seq,
    const uint32_t *flags, void *base, const uint64_t *offsets,
    const uint32_t *lens, uint64_t n, uint8_t *result, int max_devices);

/*
 * Host-memory bursts over many connections, with the payload cipher: what a
 * receive loop takes off one shared, encrypted UDP socket (datagrams in host
 * memory, of many connections, encrypted) in one synchronous call, and the
 * send side of the same loop.  `tab` (and `ctab`) are the device tables above;
 * table_stream is a stream of their device (NULL: the null stream); every
 * other pointer is host memory, each array page-locked or pageable on its own.
 * conn[i] is the slot of datagram i in both tables.  When a call returns every
 * output is complete and nothing reads or writes the caller's memory any more.
 *
 * The results are those of the device-resident calls run on one stream over
 * the same bytes, bit for bit:
 *   RX: net2_packet_decode_burst_mc(tab, conn, ivlen, ...), then, with ctab,
 *   net2_packet_decrypt_burst_mc(ctab, conn, hashlen of tab's row, ..., out,
 *   plen).  result, iv (may be NULL), seq / flags (both or neither) and plen
 *   are what that sequence leaves.  The first plen[i] bytes at out +
 *   offsets[i] + po(i) of a decrypted datagram are its plaintext; what follows
 *   them within that datagram's own bytes of `out` is unspecified, and no
 *   other byte of `out` changes value.  out == base decrypts in place; any
 *   other `out` must not overlap the burst.
 *   TX: with ctab, net2_ph_to_iv_dev(seq, flags, n, 16, ...) and
 *   net2_packet_encrypt_burst_mc(ctab, conn, hashlen, ..., plen, ..., wire_len)
 *   -- slot i = base[offsets[i] .. + lens[i]) holding plen[i] plaintext bytes
 *   at po(i) -- then net2_packet_encode_burst_mc with wire_len as its lengths.
 *   result[i] is the cipher step's code where that is not NET2_PENCODE_OK,
 *   else the hash step's; every byte of the caller's buffer is as the sequence
 *   leaves the device copy (bytes between the slots keep their value).
 *   ctab == NULL: the hash step alone -- the host forms of
 *   net2_packet_{decode,encode}_burst_mc.  lens are the datagram lengths; RX
 *   does not look at out and plen, TX not at plen and wire_len (all may be
 *   NULL), and ivlen is any length up to 64.
 *
 * The call runs on the tables' device, which must be the calling thread's
 * current device (it still is afterwards); tables are per device, so there is
 * no max_devices and no sharding.  The datagrams go through the host bursts'
 * pipeline: 64 MiB chunks, two in flight, copied as they lie from one dense
 * page-locked allocation and packed into pinned staging otherwise; one host
 * burst -- of either kind -- runs per device at a time.  The forms of the
 * steps are those of the device calls, decided per chunk under
 * net2_sha2_burst_limits, net2_aes_burst_limits and net2_aes_encrypt_limits
 * and counted in their *_stats.
 *
 * Table updates queued on table_stream before the call are seen by it: the
 * call records one event there and its own streams wait for it (no host
 * synchronisation), so the tables' "ordered in the stream" property holds for
 * table_stream.  Updates on any other stream must have completed.
 *
 * 0; EINVAL -- all before any device work, in this order: tab NULL; ivlen > 64;
 * then for n > 0 a NULL base, offsets, lens or result, or n > UINT32_MAX; conn
 * NULL; RX seq / flags not given together, TX either missing; with ctab: ivlen
 * not 16, RX out or plen NULL, TX plen or wire_len NULL, or tables of two
 * devices -- then ENODEV (no usable current device), EINVAL (the current device
 * is not the tables'), ENOMEM or EIO (then some results may be unset, but what
 * the chunks before the failed one delivered is complete).  n == 0 is 0 and
 * touches nothing.
 */
int net2_packet_decode_burst_mc_host(const struct net2_burst_keytab *tab,
    const struct net2_burst_ciphertab *ctab /* NULL: hash step only */,
    const uint32_t *conn, uint32_t ivlen, const void *base,
    const uint64_t *offsets, const uint32_t *lens, uint64_t n,
    uint8_t *result, void *iv, uint32_t *seq, uint32_t *flags,
    void *out, uint32_t *plen, void *table_stream);
int net2_packet_encode_burst_mc_host(const struct net2_burst_keytab *tab,
    const struct net2_burst_ciphertab *ctab /* NULL: hash step only */,
    const uint32_t *conn, const uint32_t *seq, const uint32_t *flags,
    void *base, const uint64_t *offsets, const uint32_t *lens,
    const uint32_t *plen, uint64_t n, uint8_t *result, uint32_t *wire_len,
    void *table_stream);

#ifdef __cplusplus
}
#endif
#endif /* NET2_PACKET_H */
