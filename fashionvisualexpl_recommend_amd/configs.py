"""On-disk contract of the hot path: the path templates of the reference's
src/config/configs.py:2-33 (only the entries BPRMF, VBPR, GradFashion, ACF and AttentiveFashion consume).

The reference's templates are cwd-relative ('../data/{0}/', so its scripts must run
from src/).  The same relative defaults are kept; `set_roots()` lets a caller point
them elsewhere (tests, bench) without changing the working directory.
"""
import os

_data_root = os.environ.get("BPRX_DATA_ROOT", "../data")
_results_root = os.environ.get("BPRX_RESULTS_ROOT", "../results")


def set_roots(data_root=None, results_root=None):
    global _data_root, _results_root
    if data_root is not None:
        _data_root = str(data_root)
    if results_root is not None:
        _results_root = str(results_root)


def data_path(dataset):                      # configs.py:2
    return os.path.join(_data_root, dataset) + os.sep


def training_path(dataset):                  # configs.py:9
    return data_path(dataset) + "trainingset.tsv"


def validation_path(dataset):                # configs.py:10
    return data_path(dataset) + "validationset.tsv"


def test_path(dataset):                      # configs.py:11
    return data_path(dataset) + "testset.tsv"


def dataset_info(dataset):                   # configs.py:14
    return data_path(dataset) + "stats_after_downloading"


def cnn_features_path(dataset, cnn_model, output_layer):   # configs.py:12,17
    return data_path(dataset) + "original/" + "cnn_features_{0}_{1}.npy".format(cnn_model, output_layer)


def cnn_features_path_split(dataset, cnn_model, output_layer):   # configs.py:18 (ACF: one {item}.npy per item)
    return data_path(dataset) + "original/" + "features/" + "cnn_{0}_{1}/".format(cnn_model, output_layer)


def edge_features_path(dataset, cnn_model, output_layer):  # configs.py:20 (GradFashion's edge features)
    return data_path(dataset) + "original/" + "edge_features_{0}_{1}.npy".format(cnn_model, output_layer)


def hist_color_features_path(dataset):       # configs.py:23-24 (GradFashion's colour histograms)
    return data_path(dataset) + "original/" + "features/" + "histograms.npy"


def edges_path(dataset):                     # configs.py:29 (AttentiveFashion: one {item}.tiff per item)
    return data_path(dataset) + "original/" + "features/" + "edges/"


def hist_color_features_path_dir(dataset):   # configs.py:25 (AttentiveFashion: one {item}.npy per item)
    return data_path(dataset) + "original/" + "features/" + "color_histograms/"


def class_features_path_dir(dataset):        # configs.py:27 (AttentiveFashion: one {item}.npy per item)
    return data_path(dataset) + "original/" + "features/" + "one_hot_encodings/"


def weight_dir():                            # configs.py:32
    return os.path.join(_results_root, "rec_model_weights")


def results_dir():                           # configs.py:33
    return os.path.join(_results_root, "rec_results")
