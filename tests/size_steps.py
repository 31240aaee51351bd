"""The sizes at which the device sort (radix_sort.hpp, rank_order.hip) and the read pivot (read_pivot.hip) take another path,
mirrored from the sources for the tests that cross them (test_sort_scan_steps_gpu.py, test_read_pivot_steps_gpu.py).
test_pivot_ref.py reads the same constants out of the sources and compares: a change there fails that test instead of quietly
moving a case back below its step."""

# radix_sort.hpp
RS_THREADS = 256                 # kRsThreads
RS_ITEMS = 8                     # kRsItems
RS_TILE = RS_THREADS * RS_ITEMS  # kRsTile: pairs per block
RS_SCAN_CHUNK = 4096             # kRsScanChunk: histogram entries per block of the scan kernels
RS_TOPS_ROUND = 256              # rs_scan_tops_kernel: chunk sums per round of its one block (its block size)
# rank_order.hip
RANK_GRID_CAP = 8192             # blocks of 256 threads of the key / iota / emit / argsort-key kernels
# read_pivot.hip
SCAN_PER = 16                    # kScanPer
SCAN_CHUNK = 256 * SCAN_PER      # kScanChunk: entries per block of the int64 scans
SCAN_TOPS_ROUND = 256            # scan_tops_kernel: chunk sums per round
SMALL_ROW = 1024                 # kSmallRow: rows ranked in LDS; larger ones take the radix sort
WAVES = 4                        # kWaves: reads / rows per block of the wave-per-item kernels
PIVOT_GRID_CAP = 65536           # grid_for: blocks at most
DEVICE_ENCODE_ABOVE = 4_000_000  # kDeviceEncodeAbove (= detect.DEVICE_ENCODE_ABOVE)
POS_LIMIT = 1 << 40              # kPosLimit: positions are below it

RS_ONE_ROUND_MAX = RS_TOPS_ROUND * RS_SCAN_CHUNK // 256 * RS_TILE     # 8 388 608: the last n whose chunk sums fit one round
SCAN_ONE_ROUND_MAX = SCAN_TOPS_ROUND * SCAN_CHUNK                     # 1 048 576 scanned entries
RANK_ONE_SWEEP_MAX = RANK_GRID_CAP * 256                              # 2 097 152 elements
PLACE_ONE_SWEEP_MAX = PIVOT_GRID_CAP * WAVES                          # 262 144 reads


def rs_tiles(n):
    return (n + RS_TILE - 1) // RS_TILE


def rs_chunk_sums(n):
    """nb of rs_sort_pairs: the chunk sums rs_scan_tops_kernel scans"""
    return (256 * rs_tiles(n) + RS_SCAN_CHUNK - 1) // RS_SCAN_CHUNK


def scan_blocks(n):
    """scan_blocks(n) of read_pivot.hip: the chunk sums scan_tops_kernel scans"""
    return (n + SCAN_CHUNK - 1) // SCAN_CHUNK
