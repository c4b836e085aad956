"""``from Dataset import get_benchmark_stream`` as the reference's local_test.py:8 does, and ``from Dataset import
get_dataset_stream`` as its local_train.py:6 does; ``DecoySet`` writes the sets that stream reads."""
from .SplitComplexBenchmark import get_benchmark_stream, read_pdb_list, read_dataset_list, SplitComplexBenchmark
from .SplitComplexDataset import get_dataset_stream, SplitComplexDataset, BatchSamplerQuality
from .DecoySet import native_pose, near_native_poses, pose_entries, write_decoy_set
