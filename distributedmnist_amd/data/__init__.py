from .mnist_data import (DataSet, Datasets, SyntheticDataSet, load_mnist,  # noqa: F401
                         read_data_sets)
from .device_data import DeviceDataSet, load_device_mnist  # noqa: F401
