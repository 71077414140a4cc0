"""GULFPORT (MUUFL Gulfport; reference loader/GULFPORTDataLoader.py): a 64-band hyperspectral raster plus one LiDAR
band, ground truth with classes 1..11 that become labels 0..10.  No shadow map: `load_shadow_map` returns None, as the
reference's does.  Rasters: classic TIFFs in any layout common/tiff_io.py reads; with a compute backend the two scene
rasters are decoded on the device (tiff_io.read_raster), the ground truth on the host."""
import numpy

from hypelcnn_amd.common.common_nn_ops import read_targets_from_image, shuffle_test_data_using_ratio, \
    shuffle_training_data_using_ratio, shuffle_training_data_using_size
from hypelcnn_amd.common import device_scene
from hypelcnn_amd.common.device_scene import make_basic_data_set
from hypelcnn_amd.loader.DataLoader import DataLoader, SampleSet

CLASS_COLORS = [
    (0, 128, 0),      # trees
    (25, 255, 25),    # mostly grass
    (0, 255, 255),    # mixed ground surface
    (255, 204, 0),    # dirt and sand
    (255, 20, 67),    # road
    (0, 0, 204),      # water
    (102, 0, 204),    # building shadow
    (255, 132, 156),  # buildings
    (204, 102, 0),    # sidewalk
    (255, 255, 207),  # yellow curb
    (208, 45, 115),   # cloth panels
]


class GULFPORTDataLoader(DataLoader):

    def __init__(self, base_dir):
        self._base_dir = base_dir
        self._hsi_file = "muulf_hsi"
        self._lidar_file = "muulf_lidar"
        self._file_ext = ".tif"
        self.backend = None  # scene preparation: this backend, else a visible HIP device, else the host

    def get_model_base_dir(self):
        return self._base_dir + "/GULFPORT/"

    def load_data(self, neighborhood, normalize):
        return self._load_data_utility(self._hsi_file + self._file_ext, self._lidar_file + self._file_ext,
                                       neighborhood, normalize)

    def _load_data_utility(self, hsi_file, lidar_file, neighborhood, normalize, casi_min=None, casi_max=None):
        from hypelcnn_amd.common.tiff_io import read_raster
        backend = device_scene.resolve_scene_backend(self.backend)
        casi = read_raster(self.get_model_base_dir() + hsi_file, backend)
        lidar = read_raster(self.get_model_base_dir() + lidar_file, backend)[:, :, numpy.newaxis]
        return make_basic_data_set(backend, shadow_creator_dict=None, casi=casi, lidar=lidar,
                                   neighborhood=neighborhood, normalize=normalize, casi_min=casi_min,
                                   casi_max=casi_max)

    def load_samples(self, train_data_ratio, test_data_ratio):
        result = self.read_targets("muulf_gt.tif")
        if train_data_ratio < 1.0:
            train_set, validation_set = shuffle_training_data_using_ratio(result, train_data_ratio)
        else:
            train_set, validation_set = shuffle_training_data_using_size(self.get_class_count(), result,
                                                                         int(train_data_ratio), None)
        test_set, train_set = shuffle_test_data_using_ratio(train_set, test_data_ratio)
        return SampleSet(training_targets=train_set, test_targets=test_set, validation_targets=validation_set)

    def read_targets(self, target_image_path):
        from hypelcnn_amd.common.tiff_io import imread
        return self._convert_targets_aux(imread(self.get_model_base_dir() + target_image_path))

    @staticmethod
    def _convert_targets_aux(targets):
        """rows (x, y, label) of the pixels marked 1..11, class-major, with the label shifted to 0..10"""
        return read_targets_from_image(targets, range(1, 12)) - [0, 0, 1]

    def load_shadow_map(self, neighborhood, data_set):
        return None

    def get_class_count(self):
        return range(0, 11)

    def get_samples_color_list(self):
        return numpy.asarray(CLASS_COLORS, dtype=numpy.uint8)

    def get_band_measurements(self):
        return numpy.linspace(405, 1005, 64)
