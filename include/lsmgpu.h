/*
 * lsmgpu.h — C ABI of the MI355X-native SST block codec (drop-in for the
 * fjall-rs/lsm-tree 3.1.9 block build/read API; see INTEGRATION.md for the
 * Rust `extern "C"` binding a maintainer would add).
 *
 * All entry points are batched: one call encodes or decodes many blocks in HBM.
 * Pointers named d_* are DEVICE pointers (hipMalloc'd, or torch CUDA tensors);
 * structs are passed by host pointer and hold device pointers.  `stream` is a
 * hipStream_t (NULL = default stream).  Every call is asynchronous on `stream`
 * and returns LSM_OK once the work is enqueued, or an argument error.
 * Per-block outcomes are written to d_status[] (lsm_status codes) on device.
 *
 * Reference interfaces replaced (paths relative to the reference repo):
 *   lsm_encode_blocks(32) <- DataBlock::encode_into src/table/data_block/mod.rs:523-549
 *                         IndexBlock::encode_into  src/table/index_block/mod.rs:110-127
 *                         Block::write_into        src/table/block/mod.rs:45-84
 *                         (per-block loop of Writer::spill_block, src/table/writer/mod.rs:303-337)
 *   lsm_decode_blocks  <- Block::from_file         src/table/block/mod.rs:131-182
 *                         Block::from_reader       src/table/block/mod.rs:87-128
 *                         load_block type check    src/table/util.rs:79-86
 *                         DataBlock::iter/Decoder  src/table/data_block/mod.rs:476, block/decoder.rs:442-483
 *                         IndexBlock::iter         src/table/index_block/mod.rs:91-95
 *   lsm_cut_blocks     <- Writer::write chunking   src/table/writer/mod.rs:243-296
 *   lsm_cut_blocks_device <- the same rule on device offsets  src/table/writer/mod.rs:284-290,374
 *                         PartitionedIndexWriter::register_data_block's partition cut
 *                                                   src/table/writer/index/partitioned.rs:166-179
 *   lsm_index_entries  <- KeyedBlockHandle of each spilled block  src/table/writer/mod.rs:332-337
 *                         FullIndexWriter           src/table/writer/index/full.rs:55-69
 *                         PartitionedIndexWriter (partitions, TLI)  src/table/writer/index/partitioned.rs:54-201
 *   lsm_xxh3_128_batch <- hash128                  src/hash.rs:7-9 (checksum of arbitrary byte ranges)
 *   lsm_point_read_blocks <- DataBlock::point_read src/table/data_block/mod.rs:412-472
 *   lsm_seek_blocks    <- data_block::Iter::seek / seek_upper (+ _exclusive)  data_block/iter.rs:37-176
 *   lsm_xxh3_128_file  <- ChecksummedWriter         src/checksum.rs:59-96 (whole-file checksum)
 *   lsm_xxh3_128_stream_{init,update,digest}
 *                      <- ChecksummedWriter::{new,write,checksum} src/checksum.rs:59-96 (streaming)
 *   lsm_xxh3_128_stream_{init,update,digest}_batch
 *                      <- the same for every table of a MultiWriter  src/table/multi_writer.rs:181-257
 *   lsm_lz4_decompress_blocks <- Block::from_reader/from_file, CompressionType::Lz4  block/mod.rs:87-182
 *   lsm_lz4_plan_output <- the builder_unzeroed(uncompressed_length) sizing of the same  block/mod.rs:104-112
 *   lsm_lz4_plan_framed / lsm_lz4_decompress_framed + lsm_decode_blocks_tuned(LSM_DECODE_PAYLOAD_VERIFIED)
 *                      <- Block::from_reader(Lz4) then DataBlock::new + iter   block/mod.rs:104-118, data_block/mod.rs:335,476
 *   lsm_lz4_compress_blocks <- Block::write_into with CompressionType::Lz4  block/mod.rs:60-74
 *   lsm_materialize_plan / lsm_materialize_keys <- DataBlockParsedItem::materialize  data_block/mod.rs:296-315
 *   lsm_materialize_items_plan / lsm_materialize_items
 *                      <- the same producing the owned InternalValue (key and value) that Scanner::next
 *                         yields (scanner.rs:74-92) into Merger::new (compaction/worker.rs:149-182)
 *   lsm_scan_table     <- Scanner::new / next      src/table/scanner.rs:24-92 (block handles from the
 *                         block index: FullBlockIndex / TwoLevelBlockIndex, src/table/block_index/,
 *                         regions from the TOC, src/table/regions.rs:55-76)
 *   lsm_table_get      <- Table::get / point_read  src/table/mod.rs:229-340 (seqno-range check, filter
 *                         block, BlockIndex::forward_reader over FullBlockIndex / TwoLevelBlockIndex,
 *                         index_block::Iter::seek index_block/iter.rs:25-34, load_data_block +
 *                         DataBlock::point_read)
 *   lsm_table_range    <- Table::range             src/table/mod.rs:391-422, the forward drain of the table
 *                         Iter src/table/iter.rs:94-293 (index seeks iter.rs:186-221, both data-block seeks
 *                         per block iter.rs:272-277), index_block::Iter::seek / seek_upper
 *                         index_block/iter.rs:25-40 over partition_point_2 block/decoder.rs:210-256,
 *                         TwoLevelBlockIndex's Iter block_index/two_level.rs:78-173
 *   lsm_table_range_rows_plan / lsm_table_range_rows
 *                      <- the items Table::range yields  src/table/mod.rs:391-422, iter.rs:272-290
 *                         (the owned InternalValue with seqno + global_seqno of every row between the two
 *                         positions of lsm_table_range)
 *   lsm_table_get_framed / lsm_table_range_framed / lsm_table_range_rows_plan_framed / lsm_table_range_rows_framed
 *                      <- the same three on a table whose data blocks are LZ4: load_block through the block
 *                         cache  src/table/util.rs:79-86, Block::from_file  block/mod.rs:131-182
 *   lsm_merge_runs     <- Merger::new / next      src/merge.rs:34-100
 *                         CompactionStream          src/compaction/stream.rs:46-221
 *                         InternalKey Ord           src/key.rs:59-72
 *                         (as composed in compaction/worker.rs:149-182,389-390)
 *   lsm_merge_read     <- TreeIter::create_range   src/range.rs:99-235 (seqno_filter range.rs:22-24,
 *                         Merger::new, MvccStream::next src/mvcc_stream.rs:45-52, the tombstone filter)
 *   lsm_bloom_shape    <- BloomConstructionPolicy::init  src/table/filter/mod.rs:25-34
 *   lsm_hash64_keys    <- FullFilterWriter::register_key src/table/writer/filter/full.rs:47-50
 *   lsm_bloom_build    <- standard_bloom Builder set_with_hash + build  builder.rs:33-53,154-170
 *   lsm_bloom_contains <- StandardBloomFilterReader::contains_hash  standard_bloom/mod.rs:100-120
 */
#ifndef LSMGPU_H
#define LSMGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LSM_ABI_VERSION 7
#define LSM_HEADER_LEN 33  /* Header::serialized_len(), header.rs:64-76 */
#define LSM_TRAILER_LEN 31 /* TRAILER_SIZE, trailer.rs:14-23 */
/* d_blocks must be 16-byte aligned and readable for LSM_INPUT_PADDING bytes
 * past the last block (vector loads stage whole 16-byte granules). */
#define LSM_INPUT_PADDING 64

/* Per-block status.  Values mirror crate::Error (src/error.rs:134-167). */
typedef enum lsm_status {
    LSM_OK = 0,
    LSM_BAD_MAGIC = 1,     /* Error::InvalidHeader("Block")           header.rs:125-127 */
    LSM_BAD_TYPE = 2,      /* Error::InvalidTag(("BlockType", v))     type.rs:33 */
    LSM_HDR_CKSUM = 3,     /* Error::ChecksumMismatch (header)        header.rs:156-161 */
    LSM_CKSUM = 4,         /* Error::ChecksumMismatch (payload)       block/mod.rs:141-149 */
    LSM_PARSE = 5,         /* malformed payload: the reference panics (lib.rs:62-66) */
    LSM_OVERFLOW = 6,      /* output capacity exceeded */
    LSM_TYPE_MISMATCH = 7, /* Error::InvalidTag, block type != expected (util.rs:81-86) */
    LSM_TRUNCATED = 8,     /* handle shorter than header / data_length mismatch (Error::Io) */
    LSM_UNSUPPORTED = 9,   /* compression != None, filter block parse */
    LSM_BAD_ARG = 10,
    LSM_HIP_ERROR = 11,
    LSM_DECOMPRESS = 12,   /* Error::Decompress(Lz4): malformed LZ4 block   block/mod.rs:113-114 */
    /* Internal hand-off mark, never the result of a completed call: a streamed
     * huge-block checksum chain (lsm_decode_blocks_tuned, LSM_DECODE_HUGE_POOL,
     * blocks >= 2 MiB) stopped waiting for the parse units of its block (no
     * progress for 5 ms, e.g. other streams' kernels holding the CUs).  The
     * call's fallback chain pass recomputes every block so marked after the
     * parse kernel has ended and overwrites the mark with the block's real
     * status; only diagnostic builds can skip that pass.  It is not a
     * checksum mismatch (block/mod.rs:141-149 reports only real mismatches). */
    LSM_INCOMPLETE = 13
} lsm_status;

/* BlockType codes, src/table/block/type.rs:13-22 */
enum { LSM_BLOCK_DATA = 0, LSM_BLOCK_INDEX = 1, LSM_BLOCK_FILTER = 2, LSM_BLOCK_META = 3 };
/* ValueType codes, src/value_type.rs:36-58 */
enum { LSM_VALUE = 0, LSM_TOMBSTONE = 1, LSM_WEAK_TOMBSTONE = 2, LSM_INDIRECTION = 4 };

/* Encode input: the items of all blocks, in key order, as SoA arenas.
 * Item i: key = keys[key_off[i] .. key_off[i+1]), value likewise.
 * Data/meta blocks use keys, vals, seqno, vtype (InternalValue, value.rs:85-153).
 * Index blocks use keys (= end_key), seqno, handle_off, handle_size
 * (KeyedBlockHandle, index_block/block_handle.rs:67-80). */
typedef struct lsm_items {
    const uint8_t* keys;
    const uint64_t* key_off;     /* [n_items + 1] */
    const uint8_t* vals;
    const uint64_t* val_off;     /* [n_items + 1] */
    const uint64_t* seqno;       /* [n_items] */
    const uint8_t* vtype;        /* [n_items] ValueType code */
    const uint64_t* handle_off;  /* [n_items] index blocks only, else NULL */
    const uint32_t* handle_size; /* [n_items] index blocks only, else NULL */
    uint64_t n_items;
} lsm_items;

/* lsm_items with 32-bit key / value offsets (SURVEY 8(d)'s 4 + 4 bytes per item
 * instead of 8 + 8): for key and value arenas of less than 4 GiB each and fewer
 * than 2^32 - 1 items.  Same meaning, field for field; lsm_encode_blocks32. */
typedef struct lsm_items32 {
    const uint8_t* keys;
    const uint32_t* key_off;     /* [n_items + 1] */
    const uint8_t* vals;
    const uint32_t* val_off;     /* [n_items + 1] */
    const uint64_t* seqno;       /* [n_items] */
    const uint8_t* vtype;        /* [n_items] ValueType code */
    const uint64_t* handle_off;  /* [n_items] index blocks only, else NULL */
    const uint32_t* handle_size; /* [n_items] index blocks only, else NULL */
    uint64_t n_items;
} lsm_items32;

/* Decode output (mirrors DataBlockParsedItem / IndexBlockParsedItem,
 * data_block/mod.rs:272-316, index_block/mod.rs:24-62): payload-relative
 * SliceIndexes into each block's data (util.rs:26).  Item k of block b is
 * k in [item_start[b], item_start[b+1]).  NULL fields are not written.
 *   key     = payload[key_off .. key_off + key_len]  (suffix when truncated)
 *   prefix  = payload[head.key_off .. + prefix_len], head = first item of the
 *             restart interval (materialize: Slice::fused(prefix, key))
 *   value   = payload[val_off .. val_off + val_len]  (val_len 0 for tombstones)
 * Index blocks: vtype = 0, prefix_len = 0, val_len = BlockHandle size,
 *   handle_off = BlockHandle offset, val_off = end of the end_key. */
typedef struct lsm_parsed_items {
    uint64_t* seqno;
    uint32_t* key_off;
    uint32_t* val_off;
    uint32_t* val_len;
    uint16_t* key_len;
    uint16_t* prefix_len;
    uint8_t* vtype;
    uint64_t* handle_off;
} lsm_parsed_items;

/* Compact decode output (lsm_decode_blocks16): the same fields with 16-bit
 * payload offsets and lengths, 19 bytes per item instead of 25.  Only data and
 * meta blocks whose payload is at most 65535 bytes (every 4 / 16 KiB-target
 * block) are decoded into it; index blocks and larger payloads get
 * LSM_UNSUPPORTED (after the header and checksum checks, before the trailer). */
typedef struct lsm_parsed_items16 {
    uint64_t* seqno;
    uint16_t* key_off;
    uint16_t* val_off;
    uint16_t* val_len;
    uint16_t* key_len;
    uint16_t* prefix_len;
    uint8_t* vtype;
} lsm_parsed_items16;

typedef struct lsm_block_params {
    uint8_t restart_interval; /* data_block_restart_interval (config default 16); forced 1 for index */
    uint8_t block_type;       /* LSM_BLOCK_DATA / LSM_BLOCK_INDEX / LSM_BLOCK_META */
    uint8_t compression;      /* 0 = CompressionType::None (the only supported value) */
    uint8_t reserved;         /* must be 0 (else LSM_BAD_ARG) */
    float hash_ratio;         /* data_block_hash_ratio (default 0.0) */
    uint32_t flags;           /* LSM_ENCODE_HUGE_POOL | LSM_ENCODE_RUN_PLAN or 0; any other bit is LSM_BAD_ARG */
} lsm_block_params;
/* Take the workspace pool of lsm_encode_workspace_size_ex: blocks whose image
 * exceeds 96 KiB are written and hashed by work units across the whole GPU.
 * Without this flag the pool is never used, whatever the workspace size; with
 * it, a workspace too small for the pool's fixed part encodes without it. */
#define LSM_ENCODE_HUGE_POOL 1u
/* Plan each 32-block run inside the write kernel (block offsets by a decoupled
 * look-back across runs) instead of a plan pass and a size scan before it.  Taken
 * for data blocks without a hash index and without the pool, 1-512 items per
 * block on average; the library also takes it by itself at >= 128 items per block
 * (16 KiB blocks of short records: faster there, slower for 4 KiB blocks).  Same
 * bytes and statuses either way, except: a run whose predecessors' offsets do not
 * arrive within 100 ms (never seen) reports LSM_INCOMPLETE for its blocks and every
 * later run's, and an item_start array that is not strictly increasing rejects the
 * blocks of the 32-block run that holds the fault. */
#define LSM_ENCODE_RUN_PLAN 2u

/* Tuning knobs for the decode kernel (0 = library default).  Any flag bit
 * other than LSM_DECODE_ITEM_START_VALID / LSM_DECODE_PAYLOAD_VERIFIED /
 * LSM_DECODE_HUGE_POOL is rejected with LSM_BAD_ARG. */
typedef struct lsm_decode_tuning {
    uint32_t blocks_per_wave;  /* consecutive blocks one workgroup owns (1..63, default 54) */
    uint32_t stage_bytes;      /* LDS stage bytes (256..65536, default 34560); larger blocks take the general path */
    uint32_t tile_items;       /* items one stage may hold (default 480, at most 8192) */
    uint32_t flags;            /* LSM_DECODE_ITEM_START_VALID: d_item_start already holds the
                                  prefix sum of this batch (skip the count + scan pass) */
} lsm_decode_tuning;
#define LSM_DECODE_ITEM_START_VALID 1u
/* The payload checksums were verified upstream: skip the xxh3_128 of every
 * payload (header fields, data_length, type, trailer and records are still
 * checked).  For LZ4 blocks decompressed by lsm_lz4_decompress_framed, whose
 * stored bytes Block::from_reader verified before decompressing
 * (block/mod.rs:94-118); their frame headers carry the STORED checksum. */
#define LSM_DECODE_PAYLOAD_VERIFIED 2u
/* Take the workspace pool of lsm_decode_workspace_size_ex: blocks larger than
 * 72 KiB are cut into work units across the whole GPU.  Without this flag the
 * pool is never used, whatever the workspace size (lsm_decode_blocks, which
 * takes no tuning, never uses it); with it, the pool is used when the
 * workspace holds round_up(lsm_decode_workspace_size(n_blocks), 256) + 8704
 * bytes or more (smaller: decoded without it; a pool too small for every
 * huge block leaves the rest on the one-workgroup path). */
#define LSM_DECODE_HUGE_POOL 4u

/* Point-read results (DataBlock::point_read -> Option<InternalValue>,
 * data_block/mod.rs:412-472), one row per query; NULL fields other than item
 * are not written.  item = index of the hit in its block's item order (the
 * row lsm_decode_blocks gives it), -1 = None.  For a hit the key equals the
 * needle; the value is payload[val_off .. val_off + val_len). */
typedef struct lsm_point_result {
    int32_t* item;
    uint64_t* seqno;
    uint32_t* val_off;
    uint32_t* val_len;
    uint8_t* vtype;
} lsm_point_result;

int lsm_abi_version(void);
const char* lsm_status_name(int status);
/* Last HIP error string of this thread (after LSM_HIP_ERROR). */
const char* lsm_last_error(void);
int lsm_device_count(void);
int lsm_set_device(int device);

/* ---- decode ---------------------------------------------------------------
 * Verifies and parses n_blocks on-disk blocks (header || payload) located at
 * d_blocks[d_block_off[b] .. d_block_off[b+1]) (d_block_off: n_blocks+1
 * device u64, the BlockHandle offsets/sizes).  expect_type: block type every
 * block must have (util.rs:81-86), or -1 for any.  Writes d_item_start
 * (n_blocks+1 u32: prefix sum of the trailers' item counts, clamped at
 * item_cap), the parsed items, and d_status[n_blocks].  The rows
 * [d_item_start[b], d_item_start[b+1]) of a block whose d_status is not LSM_OK
 * are unspecified (blocks larger than the LDS stage are parsed chunk by chunk
 * while their checksum is still being computed, so a block that then fails it
 * may have rows written): as in the reference, where Block::from_file returns
 * Err and no item is yielded, a caller uses no row of a failed block.
 * d_workspace: lsm_decode_workspace_size(n_blocks) bytes of device memory, or,
 * with LSM_DECODE_HUGE_POOL in tuning->flags, lsm_decode_workspace_size_ex(n_blocks,
 * blocks_bytes) bytes (blocks_bytes >= the bytes the batch spans): then blocks
 * larger than 72 KiB (the writer's up-to-4-MiB data blocks, writer/mod.rs:193-198;
 * full block indexes) are cut into work units across the whole GPU instead of one
 * workgroup each.  Same outputs and statuses either way.  The pool is taken only
 * when the flag asks for it, never from the workspace size alone. */
size_t lsm_decode_workspace_size(uint32_t n_blocks);
size_t lsm_decode_workspace_size_ex(uint32_t n_blocks, uint64_t blocks_bytes);
int lsm_decode_blocks(const uint8_t* d_blocks, const uint64_t* d_block_off, uint32_t n_blocks,
                      int32_t expect_type, const lsm_parsed_items* d_out, uint64_t item_cap,
                      uint32_t* d_item_start, int32_t* d_status, void* d_workspace,
                      size_t workspace_bytes, void* stream);
int lsm_decode_blocks_tuned(const uint8_t* d_blocks, const uint64_t* d_block_off, uint32_t n_blocks,
                            int32_t expect_type, const lsm_parsed_items* d_out, uint64_t item_cap,
                            uint32_t* d_item_start, int32_t* d_status, void* d_workspace,
                            size_t workspace_bytes, const lsm_decode_tuning* tuning, void* stream);
/* lsm_decode_blocks_tuned into the compact 19 B/item layout (lsm_parsed_items16;
 * tuning may be NULL).  Same statuses, plus LSM_UNSUPPORTED for index blocks
 * and payloads over 65535 bytes.  Replaces the same decoder.rs:442-483 /
 * data_block/mod.rs:272-316 walk as lsm_decode_blocks. */
int lsm_decode_blocks16(const uint8_t* d_blocks, const uint64_t* d_block_off, uint32_t n_blocks,
                        int32_t expect_type, const lsm_parsed_items16* d_out, uint64_t item_cap,
                        uint32_t* d_item_start, int32_t* d_status, void* d_workspace, size_t workspace_bytes,
                        const lsm_decode_tuning* tuning, void* stream);

/* ---- encode ---------------------------------------------------------------
 * Encodes n_blocks blocks; block b holds items [d_block_item_start[b],
 * d_block_item_start[b+1]) (n_blocks+1 device u32; every block non-empty,
 * mod.rs:530).  A d_block_item_start that is not strictly increasing is a
 * caller error: it gets LSM_BAD_ARG for some or all blocks of the batch (the
 * blocks planned together with the offending ones; every block when the batch
 * is planned item-parallel, >= 4 Ki items per block on average), so a caller
 * treats any LSM_BAD_ARG block as failing the whole batch.  Output blocks (header || payload) are packed back to back
 * into d_out; d_block_off (n_blocks+1 device u64) receives their offsets.
 * d_out needs lsm_encode_bound(...) bytes (status LSM_OVERFLOW otherwise).
 * d_workspace: lsm_encode_workspace_size(n_items, n_blocks) bytes, or, with
 * LSM_ENCODE_HUGE_POOL in params->flags, lsm_encode_workspace_size_ex(n_items,
 * n_blocks, out_cap) bytes: then blocks whose image exceeds 96 KiB (the writer's
 * up-to-4-MiB data blocks, writer/mod.rs:193-198) are written and hashed by work
 * units across the whole GPU instead of one workgroup each.  Same bytes either
 * way. */
uint64_t lsm_encode_bound(uint64_t n_items, uint32_t n_blocks, uint64_t key_bytes, uint64_t val_bytes,
                          const lsm_block_params* params);
size_t lsm_encode_workspace_size(uint64_t n_items, uint32_t n_blocks);
size_t lsm_encode_workspace_size_ex(uint64_t n_items, uint32_t n_blocks, uint64_t out_cap);
int lsm_encode_blocks(const lsm_items* d_items, const uint32_t* d_block_item_start, uint32_t n_blocks,
                      const lsm_block_params* params, uint8_t* d_out, uint64_t out_cap,
                      uint64_t* d_block_off, int32_t* d_status, void* d_workspace,
                      size_t workspace_bytes, void* stream);
/* lsm_encode_blocks over lsm_items32 (u32 key / value offsets): the same
 * kernels, bytes, statuses and workspace sizes; the item SoA the plan and write
 * passes read shrinks from 25 to 17 bytes per item. */
int lsm_encode_blocks32(const lsm_items32* d_items, const uint32_t* d_block_item_start, uint32_t n_blocks,
                        const lsm_block_params* params, uint8_t* d_out, uint64_t out_cap,
                        uint64_t* d_block_off, int32_t* d_status, void* d_workspace,
                        size_t workspace_bytes, void* stream);

/* ---- host-side helpers (no device work) ------------------------------------
 * Writer chunking on HOST arrays: cut a block when the running
 * sum(key_len + value_len) >= block_size (writer/mod.rs:284-290), the last
 * partial chunk is flushed as its own block (writer/mod.rs:374).  key_off and
 * val_off are host [n_items+1] arrays.  Writes block_item_start
 * (cap_blocks+1 entries) and returns the number of blocks. */
uint64_t lsm_cut_blocks(const uint64_t* key_off, const uint64_t* val_off, uint64_t n_items,
                        uint32_t block_size, uint32_t* block_item_start, uint64_t cap_blocks);

/* ---- checksums --------------------------------------------------------------
 * xxh3_128 (hash128, src/hash.rs:7-9) of n byte ranges
 * d_data[d_off[i] .. d_off[i+1]) into d_out (2 u64 per range: low, high). */
int lsm_xxh3_128_batch(const uint8_t* d_data, const uint64_t* d_off, uint32_t n, uint64_t* d_out,
                       void* stream);
/* Whole-file checksum: xxh3_128 of d_data[0 .. len) into d_out[0] (low), d_out[1]
 * (high), spread over the whole GPU (per-KiB contributions in parallel, then
 * the scramble chains: 8 waves, one accumulator each).  Replaces
 * ChecksummedWriter's streaming digest over an SST file held whole in HBM
 * (src/checksum.rs:59-96; equal to the one-shot xxh3_128,
 * tests/table_full_file_checksum.rs:26-31).  d_data readable up to 16 bytes
 * past len; workspace (16-byte aligned, any len incl. 0):
 * lsm_xxh3_128_file_workspace_size(len) bytes. */
size_t lsm_xxh3_128_file_workspace_size(uint64_t len);
int lsm_xxh3_128_file(const uint8_t* d_data, uint64_t len, uint64_t* d_out, void* d_workspace,
                      size_t workspace_bytes, void* stream);
/* The same checksum as a resumable stream, for a writer that emits the file
 * piece by piece (ChecksummedWriter::write per flushed region: data blocks,
 * then index, filter, meta and TOC, src/table/writer/mod.rs:66,99-102):
 *   init    ChecksummedWriter::new: a fresh running state in d_state
 *           (device memory, 16-byte aligned, lsm_xxh3_128_stream_state_size()
 *           bytes, caller-owned);
 *   update  ChecksummedWriter::write (checksum.rs:92-95): feed d_data[0 .. len)
 *           (device, any alignment, readable 16 bytes past len); workspace
 *           lsm_xxh3_128_stream_workspace_size(len) bytes, free again when
 *           the call's work on `stream` has finished;
 *   digest  ChecksummedWriter::checksum (Xxh3Default::digest128): xxh3_128 of
 *           everything fed so far into d_out[0..2] (low, high); the state is
 *           not changed, so updates may continue.
 * Any split of the input into updates gives the one-shot xxh3_128 of the
 * concatenation.  All three are asynchronous on `stream`; calls on one state
 * must be ordered (same stream, or events). */
size_t lsm_xxh3_128_stream_state_size(void);
size_t lsm_xxh3_128_stream_workspace_size(uint64_t len);
int lsm_xxh3_128_stream_init(void* d_state, void* stream);
int lsm_xxh3_128_stream_update(void* d_state, const uint8_t* d_data, uint64_t len, void* d_workspace,
                               size_t workspace_bytes, void* stream);
int lsm_xxh3_128_stream_digest(const void* d_state, uint64_t* d_out, void* stream);
/* The same for n running states at once (a flush or compaction that rotates
 * through several tables, src/table/multi_writer.rs:181-257, each with its own
 * ChecksummedWriter): d_states holds n states back to back (n *
 * lsm_xxh3_128_stream_state_size() bytes, 16-byte aligned, caller-owned).
 *   init_batch    ChecksummedWriter::new for every state;
 *   update_batch  state i is fed d_data[d_off[i] .. d_off[i+1]) (d_off: n+1
 *                 device u64, non-decreasing; empty ranges allowed; every
 *                 state at most once per call; the arena readable 16 bytes
 *                 past each range) in one launch sequence: the per-KiB
 *                 contributions of every state across the GPU, then 8 scramble
 *                 chains per state side by side.  total_len >= d_off[n] - d_off[0]
 *                 sizes the workspace (lsm_xxh3_128_stream_batch_workspace_size(n,
 *                 total_len) bytes, 16-byte aligned).  d_status[i] (device i32):
 *                 LSM_OK, or LSM_BAD_ARG for a state that was never initialised or
 *                 a decreasing range (that state is left unchanged); if the ranges
 *                 hold more bytes than total_len every state is LSM_BAD_ARG and
 *                 none is changed;
 *   digest_batch  d_out[2i], d_out[2i+1] = digest of state i (low, high). */
int lsm_xxh3_128_stream_init_batch(void* d_states, uint32_t n, void* stream);
size_t lsm_xxh3_128_stream_batch_workspace_size(uint32_t n, uint64_t total_len);
int lsm_xxh3_128_stream_update_batch(void* d_states, uint32_t n, const uint8_t* d_data, const uint64_t* d_off,
                                     uint64_t total_len, int32_t* d_status, void* d_workspace,
                                     size_t workspace_bytes, void* stream);
int lsm_xxh3_128_stream_digest_batch(const void* d_states, uint32_t n, uint64_t* d_out, void* stream);

/* ---- point read -----------------------------------------------------------
 * Batched DataBlock::point_read(needle, snapshot_seqno) (data_block/mod.rs:412-472),
 * the per-block step of Table::point_read (src/table/mod.rs:325-327): query q
 * looks up needle q (d_needles[d_needle_off[q] .. d_needle_off[q+1]), arena
 * readable LSM_INPUT_PADDING bytes past its end) in block d_query_block[q] of
 * the batch (same layout as lsm_decode_blocks; blocks of type Data or Meta, as
 * loaded and checksum-verified by Block::from_file).  Hash-index probe, else
 * restart binary search, then the MVCC linear scan (newest version with
 * seqno < snapshot).  d_status[q]: LSM_OK (hit or miss), or the structural
 * error of the block (LSM_PARSE, LSM_TRUNCATED, LSM_TYPE_MISMATCH, ...). */
int lsm_point_read_blocks(const uint8_t* d_blocks, const uint64_t* d_block_off, uint32_t n_blocks,
                          const uint32_t* d_query_block, const uint8_t* d_needles,
                          const uint64_t* d_needle_off, const uint64_t* d_snapshot, uint32_t n_queries,
                          const lsm_point_result* d_out, int32_t* d_status, void* stream);

/* ---- range seek ------------------------------------------------------------
 * Batched data-block iterator bounds: Iter::seek / seek_exclusive (lower bound)
 * and Iter::seek_upper / seek_upper_exclusive (upper bound),
 * src/table/data_block/iter.rs:37-176 over Decoder::partition_point
 * (block/decoder.rs:153-207), the per-block step of Table::range
 * (src/table/mod.rs:391-422).  Query q seeks block d_query_block[q] (same
 * buffer rules as lsm_point_read_blocks) with the lower bound
 * d_lo[d_lo_off[q] .. d_lo_off[q+1]) and the upper bound
 * d_hi[d_hi_off[q] .. d_hi_off[q+1]) (arenas 16-byte aligned, readable
 * LSM_INPUT_PADDING bytes past their end), d_flags[q] saying which apply.
 * Result: items [d_first[q], d_end[q]) in block order (the rows
 * lsm_decode_blocks gives them) are exactly what next(), next_back() or any
 * mix of them yields; d_found[q] bit 0 / bit 1 = the return value of the lower
 * / upper seek (needle present, or for the exclusive forms: an item beyond
 * it).  d_status[q] as for lsm_point_read_blocks. */
#define LSM_SEEK_LO 1u            /* apply the lower bound */
#define LSM_SEEK_HI 2u            /* apply the upper bound */
#define LSM_SEEK_LO_EXCLUSIVE 4u  /* seek_exclusive: skip keys equal to the lower bound */
#define LSM_SEEK_HI_EXCLUSIVE 8u  /* seek_upper_exclusive: skip keys equal to the upper bound */
int lsm_seek_blocks(const uint8_t* d_blocks, const uint64_t* d_block_off, uint32_t n_blocks,
                    const uint32_t* d_query_block, const uint8_t* d_lo, const uint64_t* d_lo_off,
                    const uint8_t* d_hi, const uint64_t* d_hi_off, const uint8_t* d_flags, uint32_t n_queries,
                    uint32_t* d_first, uint32_t* d_end, uint8_t* d_found, int32_t* d_status, void* stream);

/* ---- standard Bloom filter (src/table/filter/standard_bloom/) ---------------
 * The filter is the exact byte image of Builder::build (builder.rs:33-53):
 * "LSM\x03", filter type 0 (StandardBloom), hash type 0, m u64 LE, k u64 LE,
 * then m/8 bit bytes (bit i = byte i/8, mask 0x80 >> i%8,
 * bit_array/builder.rs:8-11).  Double hashing: h2 = (h1 >> 32) * 0x517cc1b727220a95,
 * position i = h1 % m, h1 += h2, h2 *= i for i = 1..k (builder.rs:10-13,154-170). */
enum { LSM_BLOOM_BITS_PER_KEY = 0, LSM_BLOOM_FP_RATE = 1 }; /* BloomConstructionPolicy */
#define LSM_BLOOM_HEADER 22
#define LSM_BLOOM_MAX_K 65536         /* larger k is rejected (bounded device loops) */
#define LSM_BLOOM_BAD_FILTER 0xFF     /* lsm_bloom_contains output: InvalidHeader("BloomFilter") */
/* Builder::calculate_m (builder.rs:128-151), f32 arithmetic as in the reference. */
uint64_t lsm_bloom_calculate_m(uint64_t n, float fpr);
/* (m, k) of BloomConstructionPolicy::{BitsPerKey(value), FalsePositiveRate(value)}.init(n)
 * (filter/mod.rs:25-34; with_bpk builder.rs:91-126, with_fp_rate :58-85).
 * LSM_BAD_ARG where the reference asserts (n == 0, bpk <= 0). */
int lsm_bloom_shape(uint64_t n, int policy, float value, uint64_t* m, uint64_t* k);
/* Byte length of the filter image: LSM_BLOOM_HEADER + m/8. */
uint64_t lsm_bloom_filter_size(uint64_t m);
/* hash64 = xxh3_64 (src/hash.rs:2-4) of n keys d_keys[d_key_off[i] .. d_key_off[i+1])
 * into d_out[i] (the FullFilterWriter hash buffer, writer/filter/full.rs:47-50).
 * d_keys 16-byte aligned and readable LSM_INPUT_PADDING bytes past its end. */
int lsm_hash64_keys(const uint8_t* d_keys, const uint64_t* d_key_off, uint64_t n, uint64_t* d_out, void* stream);
/* Builds the filter image of n hashes into d_filter (4-byte aligned, filter_cap >=
 * lsm_bloom_filter_size(m) rounded up to 4; the bytes past the image are zeroed).
 * m must be a positive multiple of 8 (both policies produce a multiple of 8; BitsPerKey < 1
 * gives m = 0, where the reference panics in h1 % m), 1 <= k <= LSM_BLOOM_MAX_K. */
int lsm_bloom_build(const uint64_t* d_hashes, uint64_t n, uint64_t m, uint64_t k, uint8_t* d_filter,
                    uint64_t filter_cap, void* stream);
/* d_out[i] = 1 if hash i may be contained, 0 if not (no false negatives),
 * LSM_BLOOM_BAD_FILTER if the image's header is malformed or truncated. */
int lsm_bloom_contains(const uint8_t* d_filter, uint64_t filter_len, const uint64_t* d_hashes, uint64_t n,
                       uint8_t* d_out, void* stream);

/* ---- LZ4 block decompression ----------------------------------------------
 * Block::from_reader / from_file with CompressionType::Lz4 (block/mod.rs:87-182),
 * batched: on-disk blocks d_blocks[d_block_off[b] .. d_block_off[b+1]) (header +
 * LZ4-compressed payload; same buffer rules as lsm_decode_blocks) are checked
 * (magic, type, header checksum, data_length, xxh3_128 of the stored payload) and
 * decompressed (lz4_flex::decompress_into, LZ4 block format) into
 * d_out[d_out_off[b] .. d_out_off[b+1]), whose length must be the header's
 * uncompressed_length (else LSM_OVERFLOW).  d_status[b]: LSM_OK, a header/checksum
 * status as in lsm_decode_blocks, or LSM_DECOMPRESS (malformed LZ4 stream, or one
 * that does not decode to exactly uncompressed_length bytes).
 * Workspace: lsm_lz4_workspace_size(n_blocks) bytes. */
size_t lsm_lz4_workspace_size(uint32_t n_blocks);
/* Output plan for lsm_lz4_decompress_blocks: d_out_off (n_blocks+1 device u64)
 * = exclusive prefix sum of each block's uncompressed_length, counted only for
 * blocks whose header verifies (magic, type, header checksum, data_length ==
 * handle size) and whose uncompressed_length <= max_block_bytes; other blocks
 * get 0 bytes (their decompress status is then the header error, or
 * LSM_OVERFLOW).  So a corrupt header cannot size the output, as
 * Block::from_reader allocates only after Header::decode_from passed
 * (block/mod.rs:91-112).  Workspace: lsm_lz4_plan_workspace_size(n_blocks). */
size_t lsm_lz4_plan_workspace_size(uint32_t n_blocks);
int lsm_lz4_plan_output(const uint8_t* d_blocks, const uint64_t* d_block_off, uint32_t n_blocks,
                        uint64_t max_block_bytes, uint64_t* d_out_off, void* d_workspace, size_t workspace_bytes,
                        void* stream);
int lsm_lz4_decompress_blocks(const uint8_t* d_blocks, const uint64_t* d_block_off, uint32_t n_blocks,
                              uint8_t* d_out, const uint64_t* d_out_off, int32_t* d_status,
                              void* d_workspace, size_t workspace_bytes, void* stream);

/* LZ4 -> parse chaining.  lsm_lz4_plan_framed is lsm_lz4_plan_output with 33
 * more bytes per verified block; lsm_lz4_decompress_framed writes each block
 * as a frame d_out[d_out_off[b] ..) = Header' || decompressed payload, where
 * Header' = the stored header with data_length = uncompressed_length and its
 * header checksum recomputed (the payload checksum field stays the STORED
 * bytes' checksum).  The frames are then decoded in place with
 * lsm_decode_blocks_tuned(d_out, d_out_off, ..., flags LSM_DECODE_PAYLOAD_VERIFIED);
 * a block's final status is its lsm_lz4_decompress_framed status if that is
 * not LSM_OK, else its decode status. */
int lsm_lz4_plan_framed(const uint8_t* d_blocks, const uint64_t* d_block_off, uint32_t n_blocks,
                        uint64_t max_block_bytes, uint64_t* d_out_off, void* d_workspace, size_t workspace_bytes,
                        void* stream);
int lsm_lz4_decompress_framed(const uint8_t* d_blocks, const uint64_t* d_block_off, uint32_t n_blocks,
                              uint8_t* d_out, const uint64_t* d_out_off, int32_t* d_status,
                              void* d_workspace, size_t workspace_bytes, void* stream);
/* lsm_lz4_plan_output (framed = 0) / lsm_lz4_plan_framed (framed = 1) for an output
 * arena the caller sized without reading the plan back (no host synchronisation):
 * when the planned bytes exceed out_cap every range is left empty, so the
 * decompress writes nothing and reports LSM_OVERFLOW for each block whose header
 * verifies (grow the arena and repeat). */
int lsm_lz4_plan_capped(const uint8_t* d_blocks, const uint64_t* d_block_off, uint32_t n_blocks,
                        uint64_t max_block_bytes, int framed, uint64_t out_cap, uint64_t* d_out_off,
                        void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- LZ4 block compression --------------------------------------------------
 * Block::write_into(.., CompressionType::Lz4) (block/mod.rs:60-74), batched, as a
 * stage of its own after lsm_encode_blocks (which keeps writing
 * CompressionType::None).  Input block b is d_blocks[d_block_off[b] ..
 * d_block_off[b+1]) = Header(33) || payload exactly as lsm_encode_blocks wrote it
 * (same buffer rules as lsm_decode_blocks).  Output block b is Header' || the LZ4
 * block-format stream of the payload, where Header' has the same magic and block
 * type, data_length = the stream's length, uncompressed_length = the payload's
 * length, checksum = xxh3_128 of the stream and the header checksum recomputed.
 * Output blocks are packed back to back from offset 0 of d_out; d_out_off
 * (n_blocks+1 device u64) receives their offsets and can be handed to
 * lsm_index_entries as its d_block_off.
 *  - Always LZ4, also where the stream is longer than the payload (lz4_flex has no
 *    stored fallback; the compression type belongs to the table).  An empty payload
 *    gives the one-byte stream 00.
 *  - The stream is a conforming LZ4 block (offsets 1..65535, matches >= 4 bytes, the
 *    last sequence literals only, the last 5 bytes literals, no match starting in the
 *    last 12 bytes), decodable by lz4_flex and liblz4 alike.  Which matches it holds
 *    is pinned by no format field; it is a pure function of the payload bytes: the
 *    same payload gives the same stream wherever it sits in the batch.
 *  - Input checks (the payload is not hashed again): a handle < 33 bytes or
 *    data_length != size - 33 -> LSM_TRUNCATED, bad magic -> LSM_BAD_MAGIC, type > 3
 *    -> LSM_BAD_TYPE, data_length != uncompressed_length (already compressed) or a
 *    payload above LZ4's 0x7E000000 input limit -> LSM_UNSUPPORTED.  d_in_status may
 *    be NULL, else it is the encoder's d_status: a block whose entry is not LSM_OK gets
 *    that status.  A rejected block occupies 0 output bytes and leaves its neighbours
 *    as they are.
 *  - lsm_lz4_compress_bound(blocks_bytes, n_blocks) is an out_cap that cannot overflow
 *    (per block 33 + len + len/255 + 16).  A block whose end would pass out_cap gets
 *    LSM_OVERFLOW and no byte of it is written; d_out_off still holds the real offsets.
 *  - Workspace: lsm_lz4_compress_workspace_size(n_blocks, blocks_bytes) bytes, 256-byte
 *    aligned, blocks_bytes = d_block_off[n_blocks] - d_block_off[0].  A block whose
 *    slot does not fit a workspace sized for fewer bytes gets LSM_BAD_ARG.
 *  - n_blocks == 0 is a no-op returning LSM_OK; NULL or misaligned buffers or a
 *    workspace below lsm_lz4_compress_workspace_size(n_blocks, 0) return LSM_BAD_ARG
 *    before any HIP call.  The call is asynchronous, does no host synchronisation and
 *    no waiting between workgroups, and can be captured into a graph on one stream. */
uint64_t lsm_lz4_compress_bound(uint64_t blocks_bytes, uint32_t n_blocks);
size_t lsm_lz4_compress_workspace_size(uint32_t n_blocks, uint64_t blocks_bytes);
int lsm_lz4_compress_blocks(const uint8_t* d_blocks, const uint64_t* d_block_off, uint32_t n_blocks,
                            const int32_t* d_in_status, uint8_t* d_out, uint64_t out_cap,
                            uint64_t* d_out_off, int32_t* d_status,
                            void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- materialize (DataBlockParsedItem::materialize, data_block/mod.rs:296-315) --
 * Owned keys of decoded items: key = Slice::fused(prefix, suffix) =
 * payload[head.key_off .. + prefix_len] || payload[key_off .. + key_len], head =
 * the item's restart head (item - item % restart_interval within its block).
 * Values stay payload sub-slices (val_off, val_len), as in the reference.  Inputs
 * are lsm_decode_blocks' outputs (key_off, key_len, prefix_len required) over the
 * same blocks; n_items = d_item_start[n_blocks].  Items of blocks whose
 * d_status is not LSM_OK get empty keys.
 * lsm_materialize_plan: d_key_out_off (n_items+1 u64) = exclusive prefix sum of
 * the key lengths (workspace: lsm_materialize_workspace_size(n_items) bytes);
 * the caller sizes d_key_out from d_key_out_off[n_items], then
 * lsm_materialize_keys writes key i to d_key_out[d_key_out_off[i] .. [i+1]). */
size_t lsm_materialize_workspace_size(uint64_t n_items);
int lsm_materialize_plan(const uint8_t* d_blocks, const uint64_t* d_block_off, uint32_t n_blocks,
                         const uint32_t* d_item_start, const int32_t* d_status, const lsm_parsed_items* d_parsed,
                         uint64_t n_items, uint64_t* d_key_out_off, void* d_workspace, size_t workspace_bytes,
                         void* stream);
int lsm_materialize_keys(const uint8_t* d_blocks, const uint64_t* d_block_off, uint32_t n_blocks,
                         const uint32_t* d_item_start, const int32_t* d_status, const lsm_parsed_items* d_parsed,
                         uint64_t n_items, const uint64_t* d_key_out_off, uint8_t* d_key_out, void* stream);
/* lsm_materialize_keys into an arena of key_cap bytes sized without reading
 * d_key_out_off[n_items] back (no host synchronisation): every key is written
 * when they fit, none otherwise; *d_result (device i32) = LSM_OK or
 * LSM_OVERFLOW.  n_items may be the parsed arrays' capacity (items past
 * d_item_start[n_blocks] have empty keys). */
int lsm_materialize_keys_capped(const uint8_t* d_blocks, const uint64_t* d_block_off, uint32_t n_blocks,
                                const uint32_t* d_item_start, const int32_t* d_status,
                                const lsm_parsed_items* d_parsed, uint64_t n_items, const uint64_t* d_key_out_off,
                                uint8_t* d_key_out, uint64_t key_cap, int32_t* d_result, void* stream);

/* ---- materialize items: decoded blocks -> merge-ready item runs -------------------
 * DataBlockParsedItem::materialize producing the owned InternalValue, key and
 * value (data_block/mod.rs:296-315), as Scanner::next yields it (scanner.rs:74-92)
 * into Merger::new (compaction/worker.rs:149-182): the parsed rows of one table are
 * appended to an lsm_items-shaped SoA (what lsm_merge_runs and lsm_encode_blocks
 * take) at a cursor held on the device.
 * Inputs: the outputs of lsm_decode_blocks / lsm_scan_table(_async) over the same
 * d_blocks (frames of lsm_lz4_decompress_framed decoded with
 * LSM_DECODE_PAYLOAD_VERIFIED included); of d_parsed, key_off, key_len, prefix_len,
 * val_off, val_len, seqno and vtype are required (else LSM_BAD_ARG).  n_items is the
 * capacity of the parsed arrays.  The block count is n_blocks, or, when d_n_blocks
 * is not NULL, the device count *d_n_blocks <= n_blocks that lsm_scan_table_async
 * leaves; entries of d_item_start / d_status past the count are never read.  The
 * row count R = min(d_item_start[count], n_items) is never read back.
 * Cursor: d_base (device u64[3], NULL = {0, 0, 0}) = the {items, key bytes, value
 * bytes} already in the outputs; d_end (device u64[3], not d_base itself) = d_base
 * plus this table's {R, key bytes, value bytes}.  Passing table t's d_end as table
 * t + 1's d_base appends the tables back to back; column 0 of a cursor array
 * u64[n_tables + 1][3] is the d_run_start of lsm_merge_runs.
 * Output row d_base[0] + i is parsed row i: key = prefix || suffix exactly as
 * lsm_materialize_keys writes it, at d_out_key_off[d_base[0] + i] = d_base[1] + the
 * key bytes of the rows before i (the entry at d_base[0] + R is d_end[1]); value =
 * payload[val_off .. val_off + val_len) at d_out_val_off likewise; seqno and vtype
 * copied.  The rows of a rejected block (d_status not LSM_OK, or a header type other
 * than Data / Meta: an index block's val_len is a handle size, not a value) get an
 * empty key, an empty value, seqno 0 and vtype 0, and so does a row whose key or
 * value range does not lie inside its block's payload (a decode never produces one;
 * a mismatched d_parsed cannot make the gather read outside d_blocks).
 * lsm_materialize_items_plan writes the offsets and d_end; *d_result (device i32) =
 * LSM_OK, or LSM_OVERFLOW when d_end[0] > out_item_cap (the offset arrays hold
 * out_item_cap + 1 entries): then no offset is written and d_end still holds the
 * real totals.  Workspace: lsm_materialize_items_workspace_size(n_items) bytes.
 * lsm_materialize_items copies keys, values, seqnos and vtypes, all rows or none:
 * *d_result = LSM_OVERFLOW and nothing is written when d_end[0] > out_item_cap,
 * d_end[1] > key_cap or d_end[2] > val_cap.  No store touches a byte of either arena
 * outside [d_base[k], d_end[k]) or a seqno / vtype entry outside
 * [d_base[0], d_end[0]).  Arenas that feed lsm_merge_runs need LSM_INPUT_PADDING
 * readable bytes past key_cap / val_cap.  One wave copies 64 consecutive rows,
 * whatever blocks they lie in; a value of 256 bytes or more is copied by its whole
 * wave (a single value is not split over waves).
 * n_items = 0 or a count of 0: d_end = d_base, LSM_OK.  Both calls are asynchronous,
 * do no host synchronisation, have no wait between workgroups and may be captured
 * into a graph on one stream. */
size_t lsm_materialize_items_workspace_size(uint64_t n_items);
int lsm_materialize_items_plan(const uint8_t* d_blocks, const uint64_t* d_block_off, uint32_t n_blocks,
                               const uint32_t* d_n_blocks, const uint32_t* d_item_start, const int32_t* d_status,
                               const lsm_parsed_items* d_parsed, uint64_t n_items, const uint64_t* d_base,
                               uint64_t* d_out_key_off, uint64_t* d_out_val_off, uint64_t out_item_cap,
                               uint64_t* d_end, int32_t* d_result, void* d_workspace, size_t workspace_bytes,
                               void* stream);
int lsm_materialize_items(const uint8_t* d_blocks, const uint64_t* d_block_off, uint32_t n_blocks,
                          const uint32_t* d_n_blocks, const uint32_t* d_item_start, const int32_t* d_status,
                          const lsm_parsed_items* d_parsed, uint64_t n_items, const uint64_t* d_base,
                          const uint64_t* d_end, const uint64_t* d_out_key_off, const uint64_t* d_out_val_off,
                          uint8_t* d_out_keys, uint64_t key_cap, uint8_t* d_out_vals, uint64_t val_cap,
                          uint64_t* d_out_seqno, uint8_t* d_out_vtype, uint64_t out_item_cap, int32_t* d_result,
                          void* stream);

/* ---- whole-table scan (Scanner, src/table/scanner.rs:24-92) -----------------
 * Decodes every data block of one table file image d_file[0 .. file_len) (16-byte
 * aligned, LSM_INPUT_PADDING readable bytes past file_len), in file order, as the
 * compaction read side does.  The block handles come from the table's block
 * index on the device: the TLI block (an index block at table->tli_off, size
 * table->tli_size: the "tli" TOC section, regions.rs:55-76) lists the data
 * blocks (FullBlockIndex, writer/index/full.rs:55-69) or, with
 * table->two_level (the TOC has an "index" section), index partitions that list
 * them (TwoLevelBlockIndex, writer/index/partitioned.rs:54-125).  The data
 * blocks must be contiguous from file offset 0 (the layout Scanner reads back to
 * back) and end inside the file.  Every item's seqno gets table->global_seqno
 * added (scanner.rs:84, wrapping).
 * Outputs: d_block_off (cap_blocks+1 u64: the data blocks, as lsm_decode_blocks
 * takes them), parsed items / d_item_start / d_status as lsm_decode_blocks
 * (block type Data expected, fetch_next_block scanner.rs:54-72),
 * *n_blocks (host) = number of data blocks, *table_status (host) = LSM_OK, or the
 * status of the first failing index block, LSM_OVERFLOW (more than cap_blocks
 * blocks or index entries), LSM_TRUNCATED (handles not contiguous from 0 or past
 * file_len) or LSM_PARSE (block count != table->block_count when non-zero,
 * the metadata's data_block_count).
 * Synchronises `stream` once per index level (the block count sizes the data
 * decode); the data decode itself is left enqueued on `stream`.
 * Workspace: lsm_scan_workspace_size(cap_blocks) bytes. */
typedef struct lsm_table_scan {
    uint64_t tli_off;       /* TLI region handle (TOC "tli" section) */
    uint32_t tli_size;
    uint32_t two_level;     /* 1: TLI entries are index partitions (TOC "index" section present) */
    uint64_t global_seqno;  /* Table::global_seqno, added to every item's seqno */
    uint64_t block_count;   /* ParsedMeta data_block_count (0 = not checked) */
} lsm_table_scan;
size_t lsm_scan_workspace_size(uint32_t cap_blocks);
int lsm_scan_table(const uint8_t* d_file, uint64_t file_len, const lsm_table_scan* table,
                   uint64_t* d_block_off, uint32_t cap_blocks, const lsm_parsed_items* d_out, uint64_t item_cap,
                   uint32_t* d_item_start, int32_t* d_status, uint32_t* n_blocks, int32_t* table_status,
                   void* d_workspace, size_t workspace_bytes, void* stream);
/* lsm_scan_table without host synchronisation: the entry counts stay on the
 * device and every level is launched for the caller's bounds (index_blocks_hint
 * index partitions of a two-level index, e.g. the TLI size / 4, else
 * cap_blocks; data_blocks_hint data blocks, e.g. the metadata's
 * data_block_count, else cap_blocks: keep them tight, the ranges past the real
 * counts are decoded as empty blocks; a level with more entries than its bound
 * gets LSM_OVERFLOW).  *d_n_blocks / *d_table_status (device)
 * receive what lsm_scan_table returns in *n_blocks / *table_status; a table
 * with more data blocks than the hint gets LSM_OVERFLOW.  d_item_start /
 * d_status hold data_blocks_hint (or cap_blocks) + 1 / entries: those past
 * *d_n_blocks are not meaningful.  Same workspace as lsm_scan_table. */
int lsm_scan_table_async(const uint8_t* d_file, uint64_t file_len, const lsm_table_scan* table,
                         uint64_t* d_block_off, uint32_t cap_blocks, uint32_t index_blocks_hint,
                         uint32_t data_blocks_hint, const lsm_parsed_items* d_out, uint64_t item_cap, uint32_t* d_item_start, int32_t* d_status,
                         uint32_t* d_n_blocks, int32_t* d_table_status, void* d_workspace, size_t workspace_bytes,
                         void* stream);

/* ---- point lookup in a table (Table::get, src/table/mod.rs:229-340) -----------
 * Batched Table::get(key, seqno, key_hash) on one table file image d_file[0 .. file_len)
 * (same buffer rules as lsm_scan_table): the block index is searched on the device, so
 * the caller names no data block.  table: tli_off, tli_size, two_level and global_seqno
 * as for lsm_scan_table (block_count is ignored).  filter_off / filter_size: the region
 * handle of the TOC's "filter" section, a block Header ‖ Bloom image of type
 * LSM_BLOCK_FILTER, never compressed (mod.rs:257,271); filter_size == 0 = the table
 * has no filter.  lowest_seqno: metadata.seqnos.0.  Needles and snapshots as
 * lsm_point_read_blocks (arena 16-byte aligned, readable LSM_INPUT_PADDING bytes past
 * its end).  d_key_hash: xxh3_64 of each needle, as Tree::get computes it once for every
 * table (NULL: the kernel hashes the needle, and only when there is a filter).
 * d_active: NULL = every query; else a query with d_active[q] == 0 is not processed and
 * none of its outputs is written, so a caller can walk several tables newest first
 * without a host round trip.
 * Per query, in the reference's order:
 *  1. snap' = d_snapshot[q] saturating-minus global_seqno; lowest_seqno >= snap' gives
 *     LSM_GET_SEQNO_SKIP (mod.rs:239-243);
 *  2. with a filter: the filter block's header fields and the image header are checked,
 *     contains_hash false gives LSM_GET_FILTERED (mod.rs:280-289);
 *  3. the index seek (index_block/iter.rs:25-34 over Decoder::seek(pred, true),
 *     block/decoder.rs:210-304): the first entry whose (end_key, seqno) fails
 *     end_key < needle || (end_key == needle && seqno >= snap'), by binary search over the
 *     block's binary index (2- or 4-byte steps; index blocks have restart interval 1, any
 *     other value is LSM_PARSE).  Full index (block_index/full.rs:23-30): no such entry
 *     gives LSM_GET_NO_BLOCK.  Two-level (block_index/two_level.rs:110-173): the same seek
 *     in the TLI, then in every partition from there on, handles yielded in order across
 *     partitions; a partition whose seek finds nothing ends the iteration;
 *  4. for each yielded handle (mod.rs:317-340): DataBlock::point_read with snap'; a hit
 *     gives LSM_GET_HIT; a miss where the handle's end key is greater than the needle gives
 *     LSM_GET_MISS; otherwise the next handle.  Handles exhausted: LSM_GET_MISS if a block
 *     was read, else LSM_GET_NO_BLOCK.
 * Outputs: d_out as lsm_point_read_blocks (item required; item = index of the hit in its
 * block, -1 for every non-hit; seqno = the item's seqno + global_seqno, wrapping as
 * lsm_scan_table; val_off / val_len relative to the block's payload), d_hit_block_off /
 * d_hit_block_size (either may be NULL) = the handle of the answering block, so the value
 * is file[block_off + 33 + val_off ..); d_outcome (may be NULL) = LSM_GET_*;
 * d_status[q] = LSM_OK for outcomes 1-5, else the error at which the reference's get
 * returns Err (outcome LSM_GET_NONE): LSM_BAD_MAGIC / LSM_BAD_TYPE / LSM_TRUNCATED from a
 * block header; LSM_TYPE_MISMATCH (TLI or partition not Index, data block not Data, filter
 * not Filter); LSM_PARSE (trailer or record malformed); LSM_TRUNCATED (a handle shorter than
 * a header or ending past file_len, or data_length != size - 33); LSM_UNSUPPORTED (a data or
 * index block with data_length != uncompressed_length, i.e. an LZ4 table, or a Bloom
 * k > LSM_BLOOM_MAX_K); LSM_BAD_MAGIC for a malformed Bloom image header.
 * Limits: partitioned filters (the TOC's "filter_tli") are not supported (the reference
 * leaves the unpinned form unimplemented, mod.rs:265-266); LZ4-compressed tables are
 * read by lsm_table_get_framed.  Payload checksums are not recomputed (the contract of
 * lsm_point_read_blocks: blocks as loaded by Block::from_file): verify the regions once
 * with lsm_decode_blocks or lsm_xxh3_128_batch.  No byte outside
 * d_file[0 .. file_len + LSM_INPUT_PADDING) is read, whatever the file holds.
 * Asynchronous on `stream`: no host synchronisation, no workspace.
 * LSM_BAD_ARG (before any device work): a NULL required pointer, d_file or d_needles not
 * 16-byte aligned, tli_size < 33, the TLI or the filter range outside the file. */
enum {
    LSM_GET_NONE = 0,       /* d_status[q] != LSM_OK */
    LSM_GET_SEQNO_SKIP = 1, /* the table holds nothing below the snapshot */
    LSM_GET_FILTERED = 2,   /* the Bloom filter excludes the key */
    LSM_GET_NO_BLOCK = 3,   /* the index names no block for the key */
    LSM_GET_MISS = 4,       /* a data block was read, no visible version in it */
    LSM_GET_HIT = 5
};
int lsm_table_get(const uint8_t* d_file, uint64_t file_len, const lsm_table_scan* table,
                  uint64_t filter_off, uint32_t filter_size, uint64_t lowest_seqno,
                  const uint8_t* d_needles, const uint64_t* d_needle_off, const uint64_t* d_snapshot,
                  const uint64_t* d_key_hash, const uint8_t* d_active, uint32_t n_queries,
                  const lsm_point_result* d_out, uint64_t* d_hit_block_off, uint32_t* d_hit_block_size,
                  uint8_t* d_outcome, int32_t* d_status, void* stream);

/* ---- range bounds in a table (Table::range, src/table/mod.rs:391-422) ----------
 * Batched Table::range(bounds) on one table file image d_file[0 .. file_len) (same
 * buffer rules as lsm_table_get): per query, the position of the first and of the last
 * row that a forward drain (next() only) of the range yields (table Iter,
 * src/table/iter.rs:94-293).  Both index levels are searched on the device, so the
 * caller names no block.  table: tli_off, tli_size and two_level as for lsm_scan_table;
 * global_seqno and block_count are ignored (positions carry no seqno).  Bounds and
 * d_flags exactly as lsm_seek_blocks: query q's lower bound is
 * d_lo[d_lo_off[q] .. d_lo_off[q+1]), its upper bound d_hi[d_hi_off[q] .. d_hi_off[q+1])
 * (arenas 16-byte aligned, readable LSM_INPUT_PADDING bytes past their end; none of the
 * four pointers may be NULL), d_flags[q] the LSM_SEEK_* bits; a bound whose bit is clear
 * is unbounded.
 * Per query:
 *  1. the index seeks, with seqno u64::MAX (iter.rs:196,208).  An index block (restart
 *     interval 1, else LSM_PARSE) yields its entries a..=b, none if a > b
 *     (block/decoder.rs:443-447).  With a lower bound, a = the first entry failing
 *     end_key < lo || (end_key == lo && seqno >= u64::MAX) (index_block/iter.rs:25-34);
 *     no such entry ends the index drain; without one a = 0.  With an upper bound,
 *     b = the first entry with end_key > hi, or the last entry if there is none
 *     (iter.rs:36-40 over partition_point_2, block/decoder.rs:210-256, which clamps);
 *     without one b = the last entry.  Full index: the handle list H is the TLI's span.
 *     Two-level (block_index/two_level.rs:78-173): the TLI's span names the partitions,
 *     each is loaded and spanned with the same two seeks, H is their spans in order; a
 *     partition whose lower seek finds nothing ends H, the partitions after it included;
 *  2. every handle of H is a data block (type Data), seeked with both bounds as
 *     lsm_seek_blocks does (iter.rs:272-277), the crossing clamp included: [first, end).
 *     The drain is those ranges in H order.  Versions of one user key straddle blocks (the
 *     writer cuts by size), so the first and the last block of H may yield nothing.
 * The first row is `first` of the first block of H with a non-empty range, the last row
 * `end - 1` of the last such block.  d_outcome[q] = LSM_RANGE_ROWS if there is such a
 * block, LSM_RANGE_EMPTY if H is non-empty and there is none, LSM_RANGE_NO_BLOCK if H is
 * empty.  For every outcome but LSM_RANGE_ROWS only d_outcome[q] and d_status[q] are
 * written.
 * Reading order (it decides which fault a query reports): the TLI; H forwards until a
 * block yields a row or H ends (partitions loaded as they are reached); H backwards from
 * its end until a block yields a row, at the latest down to the first row's block, which
 * is not loaded twice.  Blocks strictly between the two rows are never read: a fault in
 * them is not seen.  Walking backwards, a partition whose lower seek finds nothing counts
 * as empty; on a table whose TLI and partitions agree there is none in the TLI's span.
 * Outputs (d_out: the address of an lsm_range_result, a host struct of device arrays,
 * passed as const void*; NULL fields are not written, first_item and last_item are
 * required): the handles of the two blocks, the items' indices in their
 * blocks (last_item inclusive), and, with d_data_block_off (n_data_blocks + 1 u64, the
 * table's data-block offsets as lsm_scan_table and the table writer leave them; may be
 * NULL), the two blocks' ordinals in it, found by binary search; a handle that is not
 * exactly [off[i], off[i+1]) gives that query LSM_BAD_ARG and LSM_RANGE_NONE (the array is
 * not this table's).  The positions are the reference's on any table whose index levels
 * agree with each other; data blocks may disagree with the index.  On a table as the
 * writer writes it the drain is exactly the rows from the first to the last position in
 * file order, so with the d_item_start of a scan the answer is the row window
 * [item_start[first_block] + first_item, item_start[last_block] + last_item + 1).
 * d_status[q]: as lsm_table_get (LSM_BAD_MAGIC / LSM_BAD_TYPE / LSM_TRUNCATED from a block
 * header; LSM_TYPE_MISMATCH: TLI or partition not Index, data block not Data; LSM_PARSE:
 * trailer or record malformed; LSM_TRUNCATED: a handle shorter than a header or ending
 * past file_len, or data_length != size - 33; LSM_UNSUPPORTED: a compressed block, i.e. an
 * LZ4 table).  Payload checksums are verified upstream, as for lsm_table_get.  No byte
 * outside d_file[0 .. file_len + LSM_INPUT_PADDING) is read, whatever the file holds.
 * Asynchronous on `stream`: no host synchronisation, no workspace, capturable.
 * LSM_BAD_ARG (before any device work): a NULL required pointer (d_outcome and d_status
 * are required), d_file / d_lo / d_hi not 16-byte aligned, two_level > 1, the TLI outside
 * the file, first_block or last_block requested with d_data_block_off == NULL. */
typedef struct lsm_range_result {
    uint64_t* first_block_off;
    uint32_t* first_block_size;
    uint32_t* first_item;
    uint64_t* last_block_off;
    uint32_t* last_block_size;
    uint32_t* last_item;   /* inclusive */
    uint32_t* first_block; /* ordinals in d_data_block_off */
    uint32_t* last_block;
} lsm_range_result;
enum {
    LSM_RANGE_NONE = 0,     /* d_status[q] != LSM_OK */
    LSM_RANGE_NO_BLOCK = 1, /* the index seeks name no data block: none was loaded */
    LSM_RANGE_EMPTY = 2,    /* data blocks were loaded, none yields a row */
    LSM_RANGE_ROWS = 3
};
int lsm_table_range(const uint8_t* d_file, uint64_t file_len, const lsm_table_scan* table,
                    const uint8_t* d_lo, const uint64_t* d_lo_off, const uint8_t* d_hi, const uint64_t* d_hi_off,
                    const uint8_t* d_flags, uint32_t n_queries,
                    const uint64_t* d_data_block_off, uint32_t n_data_blocks,
                    const void* d_out /* const lsm_range_result* */, uint8_t* d_outcome, int32_t* d_status,
                    void* stream);

/* ---- rows of a range in a table (Table::range's items, iter.rs:272-290) ----------
 * The rows between the positions lsm_table_range reports, as item runs: per query the
 * owned InternalValues the forward drain yields (key, value, seqno + global_seqno, value
 * type), appended to an lsm_items-shaped SoA (what lsm_merge_runs takes) at a cursor held
 * on the device.  Only the data blocks first_block ..= last_block of each query are read,
 * so a range over several tables is lsm_table_range -> these two calls -> lsm_merge_runs
 * with nothing downloaded.
 * Inputs: d_file / file_len / table as lsm_table_range (same buffer rules; of table only
 * global_seqno is used); d_data_block_off (n_data_blocks + 1 u64, required): the table's
 * data-block offsets, block b = d_file[off[b] .. off[b+1]); pos: the address of an
 * lsm_range_positions (a host struct of device arrays [n_queries], passed as const void*,
 * every field required): lsm_table_range's d_outcome, d_status, first_block, first_item,
 * last_block and last_item for the same queries and the same d_data_block_off.
 * Rows of a query: query q is live when status[q] == LSM_OK and outcome[q] ==
 * LSM_RANGE_ROWS.  Its rows, in file order: items first_item .. of block first_block,
 * every item of each block between, items ..= last_item of block last_block (items
 * first_item ..= last_item when the two are one block).  On a table as the writer writes
 * it this is exactly the forward drain (the condition lsm_table_range states for its row
 * window); on a table whose data blocks disagree with its index it is still the rows
 * between the two positions.  Row fields: key = restart-head prefix || suffix, byte for
 * byte as lsm_materialize_items writes it (the restart head of a window's first row may
 * lie before the window); value = the payload slice, empty for tombstones; seqno = the
 * item's seqno + table->global_seqno, wrapping (iter.rs:285); vtype copied.  A query that
 * is not live gets an empty run and d_row_status[q] = its input status.
 * Output layout: the cursor exactly as lsm_materialize_items: d_base (device u64[3], NULL
 * = zeros) = {items, key bytes, value bytes} already in the outputs, d_end (device u64[3],
 * not d_base itself) = d_base plus this call's totals.  Run q is the rows
 * [d_run_start[q], d_run_start[q+1]) (n_queries + 1 u64, absolute row indices:
 * d_run_start[0] = d_base[0], d_run_start[n_queries] = d_end[0]; with a base of 0 it is
 * the d_run_start of lsm_merge_runs).  Row r's offsets are d_out_key_off[r] /
 * d_out_val_off[r]; the entry at d_end[0] holds d_end[1] / d_end[2].  No store touches an
 * arena byte outside [d_base[k], d_end[k]), a seqno or vtype entry outside
 * [d_base[0], d_end[0]) or an offset entry outside [d_base[0], d_end[0]].  Arenas that
 * feed lsm_merge_runs need LSM_INPUT_PADDING readable bytes past their caps.
 * Validation: payload checksums are verified upstream, as for lsm_table_get and
 * lsm_table_range.  No byte outside d_file[0 .. file_len + LSM_INPUT_PADDING) is read,
 * whatever the file, the offsets and the positions hold.  first_block > last_block or an
 * ordinal >= n_data_blocks: LSM_BAD_ARG for that query, no block touched.  Every touched
 * block is checked in this order: (1) the handle: off[b+1] - off[b] < 33, a handle that
 * decreases or one ending past file_len: LSM_TRUNCATED; (2) the header fields as
 * lsm_table_get's load_block: LSM_BAD_MAGIC / LSM_BAD_TYPE, a type other than Data:
 * LSM_TYPE_MISMATCH, data_length != size - 33: LSM_TRUNCATED, data_length !=
 * uncompressed_length: LSM_UNSUPPORTED; (3) the trailer: LSM_PARSE; (4) the edge items:
 * first_item (first block) or last_item (last block) >= the block's item count, or
 * first_item > last_item in a single block: LSM_BAD_ARG; (5) the records: the WHOLE block
 * must parse as lsm_decode_blocks requires (every restart interval starts where the
 * binary index says, the records end at the marker, the count is the trailer's), else
 * LSM_PARSE, so that the status does not depend on where the window lies in an edge block.
 * d_row_status[q] = LSM_OK, or the status of the lowest-ordinal touched block that has
 * one; such a query gets an EMPTY run, all or nothing (the reference's iterator returns
 * Err at that block and the caller discards the read); other queries are unaffected.
 * Capacities, without a read-back: block_cap bounds the (query, block) pairs of the call,
 * row_cap its rows; both size the workspace and the grids (launched for the caps, with
 * early exit past the device counts: keep them tight), each at most 2^32 - 2.  d_need
 * (device u64[4]) = {pairs, rows, key bytes, value bytes} of the call.  More pairs than
 * block_cap: *d_result = LSM_OVERFLOW, only d_need[0] is meaningful, d_end = d_base, every
 * run empty.  More rows than row_cap: *d_result = LSM_OVERFLOW; d_need, d_end and
 * d_run_start still hold the real totals.  Else *d_result = LSM_OK.
 * lsm_table_range_rows (same file, table, offsets, positions, caps, d_base, d_end and
 * workspace, the workspace left untouched since the plan) writes all rows or none:
 * *d_result = LSM_OVERFLOW and nothing is written when the plan overflowed, or when
 * d_end[0] > out_item_cap (the offset arrays hold out_item_cap + 1 entries),
 * d_end[1] > key_cap or d_end[2] > val_cap.
 * n_queries == 0: nothing is read, d_end = d_base, LSM_OK.  LSM_BAD_ARG (before any device
 * work): a NULL required pointer, d_file not 16-byte aligned, a cap above 2^32 - 2, a
 * workspace below lsm_table_range_rows_workspace_size(n_queries, block_cap, row_cap),
 * d_end == d_base.  Both calls are asynchronous on `stream`, do no host synchronisation,
 * have no wait between workgroups and may be captured into a graph on one stream.
 * Not built: `limit`, the reverse and mixed drains (LZ4 tables: the _framed forms below).  The MVCC read filter over
 * the rows of several tables is lsm_merge_read. */
typedef struct lsm_range_positions {
    const uint8_t* outcome;      /* LSM_RANGE_* */
    const int32_t* status;
    const uint32_t* first_block; /* ordinals in d_data_block_off */
    const uint32_t* first_item;
    const uint32_t* last_block;
    const uint32_t* last_item;   /* inclusive */
} lsm_range_positions;
size_t lsm_table_range_rows_workspace_size(uint32_t n_queries, uint64_t block_cap, uint64_t row_cap);
int lsm_table_range_rows_plan(const uint8_t* d_file, uint64_t file_len, const lsm_table_scan* table,
                              const uint64_t* d_data_block_off, uint32_t n_data_blocks,
                              const void* pos /* const lsm_range_positions* */, uint32_t n_queries,
                              uint64_t block_cap, uint64_t row_cap, const uint64_t* d_base,
                              uint64_t* d_run_start, uint64_t* d_end, uint64_t* d_need, int32_t* d_row_status,
                              int32_t* d_result, void* d_workspace, size_t workspace_bytes, void* stream);
int lsm_table_range_rows(const uint8_t* d_file, uint64_t file_len, const lsm_table_scan* table,
                         const uint64_t* d_data_block_off, uint32_t n_data_blocks,
                         const void* pos /* const lsm_range_positions* */, uint32_t n_queries,
                         uint64_t block_cap, uint64_t row_cap, const uint64_t* d_base, const uint64_t* d_end,
                         void* d_workspace, size_t workspace_bytes, uint64_t* d_out_key_off,
                         uint64_t* d_out_val_off, uint8_t* d_out_keys, uint64_t key_cap, uint8_t* d_out_vals,
                         uint64_t val_cap, uint64_t* d_out_seqno, uint8_t* d_out_vtype, uint64_t out_item_cap,
                         int32_t* d_result, void* stream);

/* ---- the readers on an LZ4 table: data blocks through inflated frames -------------
 * lsm_table_get, lsm_table_range and lsm_table_range_rows for a table whose data blocks
 * are LZ4 (the default data_block_compression_policy below level 0), the reference's
 * pattern: load_block finds the decompressed block by the handle's offset in the block
 * cache, Block::from_file verifies and decompresses on a miss (src/table/util.rs:79-86,
 * block/mod.rs:131-182).  Here the cache is fully populated up front: an lsm_table_frames
 * view (a host struct of device arrays, passed as const void*) is what
 * lsm_lz4_plan_framed + lsm_lz4_decompress_framed leave when run over the table's stored
 * data-block offsets as their d_block_off: stored_off = that d_block_off, frame_off =
 * the plan's d_out_off, frames = the decompress's d_out, frame_status = its d_status,
 * frames_len = frame_off[n_blocks].  Frame b = Header' || payload with data_length =
 * uncompressed_length and the stored checksum verified, which is what the block readers
 * accept.  Index blocks, the TLI and the filter block are read from d_file, uncompressed,
 * as by the plain calls (index_block_compression_policy is None).
 * The data-block load of a handle (off, size) the index yields, in this order (it decides
 * which fault a query reports):
 *  1. the handle lies in the file, as in the plain calls: size < 33, a wrap-around or
 *     off + size > file_len: LSM_TRUNCATED;
 *  2. the ordinal: b = the last b < n_blocks with stored_off[b] <= off, by binary search
 *     (at most ceil(log2 n_blocks) steps whatever the array holds); stored_off[b] != off,
 *     stored_off[b+1] != off + size or n_blocks == 0: LSM_BAD_ARG (the view is not this
 *     table's; lsm_table_range's rule for ordinals);
 *  3. frame_status[b] != LSM_OK: that status, the Err of Block::from_file (header,
 *     LSM_CKSUM of the stored bytes, LSM_DECOMPRESS), before the type test as in the
 *     reference;
 *  4. the frame's extent: frame_off[b+1] < frame_off[b], a frame shorter than 33 bytes or
 *     one ending past frames_len: LSM_TRUNCATED;
 *  5. the plain calls' load_block on the frame: header fields, type Data
 *     (LSM_TYPE_MISMATCH), data_length == frame size - 33 (LSM_TRUNCATED), uncompressed
 *     (LSM_UNSUPPORTED), trailer (LSM_PARSE); then the same point read / seek.
 * No byte outside d_file[0 .. file_len + LSM_INPUT_PADDING) and
 * frames[0 .. frames_len + LSM_INPUT_PADDING) is read, whatever the file and the view
 * hold.  Identity view: frames = d_file, frame_off = stored_off, frame_status = NULL,
 * frames_len = file_len over an uncompressed table gives exactly the plain calls' answers.
 * lsm_table_get_framed: lsm_table_get's parameters, then the view and d_hit_block.
 *   d_hit_block_off / d_hit_block_size report the STORED handle, d_hit_block (may be NULL)
 *   its ordinal; val_off / val_len are relative to the frame's payload, so a hit's value
 *   is frames[frame_off[hit_block] + 33 + val_off ..).  Outcomes and statuses as
 *   lsm_table_get, plus those of steps 2-4.
 * lsm_table_range_framed: lsm_table_range's parameters with (d_data_block_off,
 *   n_data_blocks) replaced by the view (required).  first_block / last_block are ordinals
 *   in stored_off (the loads' own: no second search), the handles reported are the stored
 *   ones, first_item / last_item index the decompressed blocks.
 * lsm_table_range_rows_plan_framed / lsm_table_range_rows_framed: the plain calls without
 *   d_file, file_len, d_data_block_off and n_data_blocks, the view after `table`.  Block b
 *   is frame b; positions come from lsm_table_range_framed over the same view.  Every
 *   touched block is checked as by lsm_table_range_rows with frame_status[b] first
 *   (a non-OK entry is the block's status and takes part in the lowest-ordinal rule; a
 *   value outside 1..255 counts as LSM_BAD_ARG), then (1) the handle test on frame_off
 *   against frames_len, (2)-(5) unchanged.  Row descriptors address the frame arena.
 *   Workspace size function, caps, cursor and all-or-nothing rules are the plain calls'.
 * All four are asynchronous on `stream`, do no host synchronisation, have no wait between
 * workgroups and may be captured into a graph on one stream.  LSM_BAD_ARG (before any
 * device work): a NULL view, a NULL stored_off / frames / frame_off, frames not 16-byte
 * aligned, and the plain calls' own argument errors.
 * Not built: selective inflate (the view holds every data block of the table),
 * compressed index blocks. */
struct lsm_table_frames {
    const uint64_t* stored_off;   /* device [n_blocks + 1]: the table's data-block offsets as stored in the file */
    const uint8_t*  frames;       /* device, 16-byte aligned, readable LSM_INPUT_PADDING bytes past frames_len */
    const uint64_t* frame_off;    /* device [n_blocks + 1]: frame b = frames[frame_off[b] .. frame_off[b+1]) */
    const int32_t*  frame_status; /* device [n_blocks], lsm_lz4_decompress_framed's d_status; NULL = every frame LSM_OK */
    uint64_t frames_len;          /* bytes of `frames` the kernels may read (plus the padding) */
    uint32_t n_blocks;
};
typedef struct lsm_table_frames lsm_table_frames;
int lsm_table_get_framed(const uint8_t* d_file, uint64_t file_len, const lsm_table_scan* table,
                         uint64_t filter_off, uint32_t filter_size, uint64_t lowest_seqno,
                         const uint8_t* d_needles, const uint64_t* d_needle_off, const uint64_t* d_snapshot,
                         const uint64_t* d_key_hash, const uint8_t* d_active, uint32_t n_queries,
                         const lsm_point_result* d_out, uint64_t* d_hit_block_off, uint32_t* d_hit_block_size,
                         uint8_t* d_outcome, int32_t* d_status,
                         const void* frames /* const lsm_table_frames* */, uint32_t* d_hit_block, void* stream);
int lsm_table_range_framed(const uint8_t* d_file, uint64_t file_len, const lsm_table_scan* table,
                           const uint8_t* d_lo, const uint64_t* d_lo_off, const uint8_t* d_hi,
                           const uint64_t* d_hi_off, const uint8_t* d_flags, uint32_t n_queries,
                           const void* frames /* const lsm_table_frames* */,
                           const void* d_out /* const lsm_range_result* */, uint8_t* d_outcome, int32_t* d_status,
                           void* stream);
int lsm_table_range_rows_plan_framed(const lsm_table_scan* table, const void* frames /* const lsm_table_frames* */,
                                     const void* pos /* const lsm_range_positions* */, uint32_t n_queries,
                                     uint64_t block_cap, uint64_t row_cap, const uint64_t* d_base,
                                     uint64_t* d_run_start, uint64_t* d_end, uint64_t* d_need,
                                     int32_t* d_row_status, int32_t* d_result, void* d_workspace,
                                     size_t workspace_bytes, void* stream);
int lsm_table_range_rows_framed(const lsm_table_scan* table, const void* frames /* const lsm_table_frames* */,
                                const void* pos /* const lsm_range_positions* */, uint32_t n_queries,
                                uint64_t block_cap, uint64_t row_cap, const uint64_t* d_base, const uint64_t* d_end,
                                void* d_workspace, size_t workspace_bytes, uint64_t* d_out_key_off,
                                uint64_t* d_out_val_off, uint8_t* d_out_keys, uint64_t key_cap, uint8_t* d_out_vals,
                                uint64_t val_cap, uint64_t* d_out_seqno, uint8_t* d_out_vtype,
                                uint64_t out_item_cap, int32_t* d_result, void* stream);

/* ---- merge of sorted runs with compaction GC ----------------------------------
 * CompactionStream::new(Merger::new(runs), gc_seqno_threshold)
 *     .evict_tombstones(flags & 1).zero_seqnos(flags & 2) with NoFilter
 * (merge.rs:34-100, compaction/stream.rs:46-221), the step between the
 * compaction read side and the writer (compaction/worker.rs:149-182,389-390;
 * the memtable flush uses the same pair, abstract_tree.rs:98-105).
 * Input: d_in holds every run back to back (keys, key_off, vals, val_off, seqno,
 * vtype and n_items are used; both arenas readable LSM_INPUT_PADDING bytes past
 * their end); run r is the items [d_run_start[r], d_run_start[r+1]) (n_runs + 1
 * device u64, d_run_start[0] = 0, d_run_start[n_runs] = n_items; empty runs
 * allowed), each sorted in InternalKey order (key.rs:59-72: user key ascending
 * as unsigned bytes, a key before any longer key it prefixes, then seqno
 * descending; equal neighbours are accepted).  n_items <= 2^32 - 2,
 * 1 <= n_runs <= LSM_MERGE_MAX_RUNS, no other flag bit: else LSM_BAD_ARG.
 * Output: an lsm_items-shaped SoA for lsm_cut_blocks_device / lsm_encode_blocks: item j
 * is d_out_keys[d_out_key_off[j] .. d_out_key_off[j+1]), d_out_vals likewise,
 * d_out_seqno[j], d_out_vtype[j]; entries 0 .. n_out of both offset arrays are
 * written; *d_n_out (device) = n_out; d_out_src[j] (may be NULL) = the input index
 * of output item j (the indices that never appear are the dropped items, what
 * DroppedKvCallback::on_dropped would learn of).  The caller sizes the outputs
 * for the input (n_items entries, n_items + 1 offsets, the input arenas' bytes
 * + LSM_INPUT_PADDING): the output never exceeds the input.  Outputs must not
 * overlap inputs.  Items with equal (key, seqno) in different runs (the
 * reference's heap leaves their order open) come out lower run first.
 * d_status[r] (n_runs device i32): LSM_OK, or LSM_BAD_ARG for a run that is not
 * sorted (or a malformed d_run_start); if any run is rejected *d_n_out = 0 and
 * the other outputs are unspecified.  n_items = 0 gives *d_n_out = 0.
 * No host synchronisation.  Workspace: lsm_merge_workspace_size(n_items, n_runs). */
#define LSM_MERGE_MAX_RUNS 64
#define LSM_MERGE_EVICT_TOMBSTONES 1u  /* CompactionStream::evict_tombstones(true) */
#define LSM_MERGE_ZERO_SEQNOS 2u       /* CompactionStream::zero_seqnos(true) */
size_t lsm_merge_workspace_size(uint64_t n_items, uint32_t n_runs);
int lsm_merge_runs(const lsm_items* d_in, const uint64_t* d_run_start, uint32_t n_runs,
                   uint64_t gc_seqno_threshold, uint32_t flags,
                   uint8_t* d_out_keys, uint64_t* d_out_key_off,
                   uint8_t* d_out_vals, uint64_t* d_out_val_off,
                   uint64_t* d_out_seqno, uint8_t* d_out_vtype,
                   uint32_t* d_out_src, uint64_t* d_n_out, int32_t* d_status,
                   void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- read merge: the snapshot read of per-query item runs ------------------------
 * What a reader gets from TreeIter::create_range (range.rs:99-235), for n_groups
 * queries at once: every source filtered by seqno_filter(item.seqno, snapshot)
 * (range.rs:22-24), Merger::new over the sources, MvccStream::new (the first item of
 * each user key, the rest drained, mvcc_stream.rs:45-52), then the tombstone filter.
 * The step after lsm_table_range_rows: a range over several tables is lsm_table_range
 * -> lsm_table_range_rows per table -> this call, with nothing downloaded.
 * Input: as lsm_merge_runs (d_in holds every run back to back, both arenas readable
 * LSM_INPUT_PADDING bytes past their end, n_items <= 2^32 - 2), with
 * n_sources * n_groups runs: run s * n_groups + g is source s of group (query) g,
 * source-major, the order n_sources chained lsm_table_range_rows calls over the same
 * n_groups queries write when call s is given d_run_start + s * n_groups (its last
 * entry is the next call's first).  d_run_start: n_sources * n_groups + 1 device u64,
 * first 0, last n_items, non-decreasing; empty runs are normal.  Each run is sorted in
 * InternalKey order (equal neighbours are accepted).
 * Per group g, with snap = d_group_seqno ? d_group_seqno[g] : snapshot_seqno:
 * (1) an item is visible iff seqno < snap (seqno == snap is not); (2) the visible items
 * of the group's runs are merged in InternalKey order, items with equal (key, seqno)
 * lower source first, as lsm_merge_runs; (3) of each user key only the first item of
 * that order is kept (MvccStream::next); (4) unless LSM_MERGE_READ_KEEP_TOMBSTONES is
 * set, a kept Tombstone or WeakTombstone is dropped (Indirection is kept).  The flag is
 * for a caller who merges the result with sources that stay on the host (memtables):
 * the tombstones must shadow older versions there.  MvccStream::next_back yields the
 * same items in reverse (mvcc_stream.rs test_reverse!), so the output serves both
 * directions of the iterator.
 * Output: group g's rows are [d_out_group_start[g], d_out_group_start[g+1])
 * (n_groups + 1 device u64, the first 0, the last the total), laid out as
 * lsm_merge_runs' output items; offset entries 0 ..= total are written, d_out_src[j]
 * (may be NULL) is the input index of row j, seqnos are copied unchanged.  Nothing is
 * stored past row total, past offset entry total or past the arenas' [0, last offset).
 * The caller sizes the outputs for the input, as for lsm_merge_runs.  Outputs must not
 * overlap inputs.
 * d_status[g] (n_groups device i32), per group, other groups unaffected: when
 * d_in_status (NULL or n_sources * n_groups device i32, the d_row_status of the rows
 * calls, in run order) holds a non-zero entry for a source of the group, that entry of
 * the lowest such source, and the group's output is empty (the reference's iterator
 * returns Err and the read is discarded); else LSM_BAD_ARG and an empty output when a
 * run of the group is not sorted; a malformed d_run_start gives every group
 * LSM_BAD_ARG and every d_out_group_start entry 0; else LSM_OK.
 * LSM_BAD_ARG before any device work: a NULL required pointer, n_sources outside
 * 1 ..= LSM_MERGE_MAX_RUNS, n_groups == 0 with n_items != 0, n_sources * n_groups or
 * n_items above 2^32 - 2, an unknown flag bit, a workspace below
 * lsm_merge_read_workspace_size(n_items, n_groups, n_sources).  n_groups == 0 writes
 * d_out_group_start[0] = 0.  Asynchronous on `stream`: no host synchronisation, no
 * wait between workgroups; may be captured into a graph on one stream.
 * Not built: a per-query `limit`, memtable sources, RunReader's table selection. */
#define LSM_MERGE_READ_KEEP_TOMBSTONES 1u
size_t lsm_merge_read_workspace_size(uint64_t n_items, uint32_t n_groups, uint32_t n_sources);
int lsm_merge_read(const lsm_items* d_in, const uint64_t* d_run_start,
                   uint32_t n_groups, uint32_t n_sources,
                   uint64_t snapshot_seqno, const uint64_t* d_group_seqno /* NULL or [n_groups] */,
                   const int32_t* d_in_status /* NULL or [n_sources * n_groups] */, uint32_t flags,
                   uint8_t* d_out_keys, uint64_t* d_out_key_off, uint8_t* d_out_vals, uint64_t* d_out_val_off,
                   uint64_t* d_out_seqno, uint8_t* d_out_vtype, uint32_t* d_out_src /* may be NULL */,
                   uint64_t* d_out_group_start /* [n_groups + 1] */, int32_t* d_status /* [n_groups] */,
                   void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- table write side: block cut and block index on the device -------------------
 * lsm_cut_blocks_device: lsm_cut_blocks on DEVICE offset arrays, e.g. the merge's
 * outputs.  Item i weighs key_len + val_len + extra_per_item; a block is cut after
 * the item at which the running weight reaches block_size (writer/mod.rs:284-290),
 * the last partial block is flushed (:374).  d_val_off may be NULL (weight = key
 * length + extra_per_item: with extra_per_item = size_of::<KeyedBlockHandle>() and
 * block_size = the partition size this is PartitionedIndexWriter::register_data_block's
 * rule over the index entries, partitioned.rs:166-179).  d_n_items may be NULL (n_items
 * items); else it is a device count <= n_items, such as lsm_merge_runs' d_n_out: n_items
 * is then only the arrays' capacity and entries past *d_n_items + 1 are never read.
 * Writes d_block_item_start (entries 0 .. *d_n_blocks, at most cap_blocks + 1; always
 * strictly increasing and at most the item count), *d_n_blocks (device u64) and
 * *d_status (device i32): LSM_OK; LSM_BAD_ARG for an offset array that decreases
 * (*d_n_blocks = 0); LSM_OVERFLOW for more than cap_blocks blocks (*d_n_blocks is the
 * real count, only cap_blocks + 1 starts are written).  No items: *d_n_blocks = 0,
 * d_block_item_start[0] = 0.  n_items <= 2^32 - 2, cap_blocks >= 1 with items, else
 * LSM_BAD_ARG.  No host synchronisation, no wait between workgroups; may be captured
 * into a graph.  Workspace: lsm_cut_workspace_size(n_items) bytes (8 per item). */
size_t lsm_cut_workspace_size(uint64_t n_items);
int lsm_cut_blocks_device(const uint64_t* d_key_off, const uint64_t* d_val_off, uint64_t n_items,
                          const uint64_t* d_n_items, uint32_t extra_per_item, uint32_t block_size,
                          uint32_t* d_block_item_start, uint64_t cap_blocks, uint64_t* d_n_blocks,
                          int32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream);
/* lsm_index_entries: the KeyedBlockHandles of an encoded batch (Writer::spill_block,
 * writer/mod.rs:332-337): entry b = the key and seqno of the last item of block b
 * (item d_block_item_start[b+1] - 1), handle_off = base_offset + d_block_off[b],
 * handle_size = d_block_off[b+1] - d_block_off[b], with d_block_item_start /
 * d_block_off as lsm_encode_blocks took / wrote them.  Only keys (readable
 * LSM_INPUT_PADDING bytes past the end), key_off, seqno and n_items of d_items are
 * read, so the same call over its own output and the partitions' offsets, with
 * base_offset = the index region's file offset, gives the TLI entries
 * (cut_index_block, partitioned.rs:80-84,113-115).  The outputs (d_out_key_off:
 * n_blocks + 1, the others n_blocks entries) are the index form of lsm_items and
 * feed lsm_encode_blocks with LSM_BLOCK_INDEX.  *d_result (device i32): LSM_OK, or
 * LSM_OVERFLOW when the keys exceed key_cap: then only d_out_key_off is written.
 * No host synchronisation.  Workspace: lsm_index_entries_workspace_size(n_blocks). */
size_t lsm_index_entries_workspace_size(uint32_t n_blocks);
int lsm_index_entries(const lsm_items* d_items, const uint32_t* d_block_item_start,
                      const uint64_t* d_block_off, uint32_t n_blocks, uint64_t base_offset,
                      uint8_t* d_out_keys, uint64_t key_cap, uint64_t* d_out_key_off,
                      uint64_t* d_out_seqno, uint64_t* d_out_handle_off, uint32_t* d_out_handle_size,
                      int32_t* d_result, void* d_workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LSMGPU_H */
